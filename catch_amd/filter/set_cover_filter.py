"""SetCoverFilter on the MI355X: drop-in for catch/filter/set_cover_filter.py.

Same constructor and `BaseFilter.filter()` contract as the reference class
(catch/filter/set_cover_filter.py:199-357, :902-930); the work of
`_make_sets` (:359-470), `_make_ranks` (:614-735) and
`set_cover.approx_multiuniverse` (catch/utils/set_cover.py:147-615) runs in
the HIP kernels of libcatchhip.so through `catch_amd.engine`.  There is no
CPU fallback: without the library or a GPU the filter raises.

Beyond the reference: `fixed_probes` (a trailing keyword) names probes the user
owns already; the filter then selects only what they leave uncovered
(_filter_strs_keeping_rows).  `coverage_depth` (after it) asks for every base to
be covered by that many selected probes, one greedy layer per unit of depth
(the same method).  `prune_redundant` (a keyword too) looks back at the picks
once the design is complete and drops those that cover nothing alone
(engine.Rows.prune).  `pick_gains` (a keyword) reports what every pick added
when it was taken and the coverage after the first k picks
(engine.Rows.pick_gains); `max_probes` (a keyword) keeps, over all groups, only
the N picks with the largest such gains (allocate_budget).  `target_regions` (a
keyword) says which bases are to be covered at all: after the scan the cover
rows are cut to their runs of wanted bases (engine.BaseMask, Rows.restrict), and
everything above then works on wanted bases only.  `either_strand` (a keyword)
makes a candidate cover what its own string OR its reverse complement
hybridises to: a second scan of the reverse-complemented strings against the
same targets and the union of the two row tables, set by set (Rows.union).
`max_cross_dimer` / `cross_dimer_rounds` (keywords) keep the selection, over all
groups and beside the fixed probes, free of probes that anneal to each other,
and cover again what a conflicting pick would have covered (_cross_rounds).

Not supported (raises NotImplementedError): custom hybridization functions
loaded from a Python file (`custom_cover_range_fn`, :288-299) -- an arbitrary
Python callable cannot run inside a kernel.
"""
import logging
import os

import numpy as np

from catch_amd import _lib
from catch_amd import engine
from catch_amd import probe
from catch_amd.filter.base_filter import BaseFilter
from catch_amd.utils import seq_io

logger = logging.getLogger(__name__)


def set_max_num_processes_for_set_cover_instances(max_num_processes=8):
    """catch/filter/set_cover_filter.py:66-79.  Accepted for CLI
    compatibility; set-cover instances are solved on the GPU."""
    global _sc_max_num_processes
    _sc_max_num_processes = max_num_processes


set_max_num_processes_for_set_cover_instances()

_RC = str.maketrans("ACGT", "TGCA")


def _reverse_complement(s):
    """A<->T, C<->G, everything else maps to itself (:515-521)."""
    return s[::-1].translate(_RC)


class _KeywordsBeyondInit(type):
    """SetCoverFilter(..., fixed_probes=None, coverage_depth=1,
    prune_redundant=False, max_probes=None, pick_gains=False,
    curve_points=100, target_regions=None, either_strand=False,
    max_cross_dimer=None, cross_dimer_rounds=8,
    max_cross_dimer_dg=None): everything after `fixed_probes` is a keyword of the CALL
    of the class, taken here and handed to the new object after __init__ ran.
    __init__ itself stays the reference's argument list followed by
    `fixed_probes`, the form its callers and the signature checks of the
    extension know; the others can only be given by name."""

    def __call__(cls, *args, coverage_depth=1, prune_redundant=False, max_probes=None, pick_gains=False,
                 curve_points=100, target_regions=None, either_strand=False, max_cross_dimer=None,
                 cross_dimer_rounds=8, max_cross_dimer_dg=None, **kwargs):
        obj = super().__call__(*args, **kwargs)
        obj._set_either_strand(either_strand)
        obj._set_coverage_depth(coverage_depth)
        obj._set_prune_redundant(prune_redundant)
        obj._set_budget(max_probes, pick_gains, curve_points)
        obj._set_target_regions(target_regions)
        obj._set_cross_dimer(max_cross_dimer, cross_dimer_rounds, max_cross_dimer_dg)
        return obj


class SetCoverFilter(BaseFilter, metaclass=_KeywordsBeyondInit):
    """Selects candidate probes with the greedy multi-universe set cover."""

    def __init__(self,
                 mismatches,
                 lcf_thres,
                 island_of_exact_match=0,
                 mismatches_tolerant=None,
                 lcf_thres_tolerant=None,
                 island_of_exact_match_tolerant=None,
                 custom_cover_range_fn=None,
                 custom_cover_range_tolerant_fn=None,
                 identify=False,
                 avoided_genomes=[],
                 coverage=1.0,
                 cover_extension=0,
                 kmer_probe_map_k=20,
                 kmer_probe_map_use_native_dict=False,
                 fixed_probes=None):
        if (custom_cover_range_fn is not None
                or custom_cover_range_tolerant_fn is not None):
            raise NotImplementedError(
                "custom hybridization functions cannot run on the GPU path")
        # The seed scan (cover threshold == probe length, the default) takes any
        # mismatch budget; the general path (-l below the probe length, island,
        # unequal probes, other alphabets) keeps the nearest mismatches of each
        # side in fixed arrays of 32 (csrc/scan.hip MAX_MM)
        for name, val in (("mismatches", mismatches),
                          ("mismatches_tolerant", mismatches_tolerant)):
            if val is not None and val > 32 and lcf_thres is not None:
                logger.warning("%s = %d: cover ranges below the full probe length "
                               "(-l / --island-of-exact-match) support at most 32 "
                               "mismatches on the GPU and will raise", name, val)
        self.mismatches = mismatches
        self.lcf_thres = lcf_thres
        self.island_of_exact_match = island_of_exact_match
        # tolerant parameters default to the strict ones when falsy (:308-313)
        if not mismatches_tolerant:
            mismatches_tolerant = mismatches
        if not lcf_thres_tolerant:
            lcf_thres_tolerant = lcf_thres
        if not island_of_exact_match_tolerant:
            island_of_exact_match_tolerant = island_of_exact_match
        self.mismatches_tolerant = mismatches_tolerant
        self.lcf_thres_tolerant = lcf_thres_tolerant
        self.island_of_exact_match_tolerant = island_of_exact_match_tolerant

        if identify:
            if (coverage <= 1.0 and coverage >= 0.25) or \
               (coverage > 1 and coverage >= 5000):
                logger.warning(("Identification is enabled but the required "
                                "coverage is high; generally coverage should "
                                "be small when performing identification"))
        self.identify = identify
        self.avoided_genomes = avoided_genomes
        self.coverage = coverage
        self.cover_extension = cover_extension
        self.kmer_probe_map_k = kmer_probe_map_k
        self.kmer_probe_map_use_native_dict = kmer_probe_map_use_native_dict
        self.requires_probe_groupings = True
        self._force_num_processes = None   # accepted, unused (:355-357)
        self.scan_mode = engine.SCAN_AUTO
        self.last_timings = {}
        # probes the user owns already (strings or Probe objects; not an argument of the reference's class): the
        # filter then selects only what they leave uncovered (_filter_strs_keeping_rows)
        self.fixed_probes = [q if isinstance(q, str) else q.seq_str
                             for q in (fixed_probes if fixed_probes is not None else ())]
        self.coverage_depth = 1     # (SetCoverFilter(..., coverage_depth=D) sets it: _KeywordsBeyondInit)
        self.last_layer_sizes = []
        self.prune_redundant = False   # (SetCoverFilter(..., prune_redundant=True) sets it: _KeywordsBeyondInit)
        self.last_pruned = []
        self.max_probes = None      # (SetCoverFilter(..., max_probes=N / pick_gains=True / curve_points=P): _KeywordsBeyondInit)
        self.pick_gains = False
        self.curve_points = 100
        self.last_pick_gains = []
        self.last_budget_kept = []
        self.last_coverage_curve = []
        self.target_regions = None  # (SetCoverFilter(..., target_regions=R) sets it: _KeywordsBeyondInit)
        self.last_wanted_bases = []
        self.last_coverable_bases = []
        self.either_strand = False  # (SetCoverFilter(..., either_strand=True) sets it: _KeywordsBeyondInit)
        self._strand_scan = None    # what the last _scan_group did under either_strand (_either_strand_rows)
        self.max_cross_dimer = None  # (SetCoverFilter(..., max_cross_dimer=X, cross_dimer_rounds=R): _KeywordsBeyondInit)
        self.max_cross_dimer_dg = None
        self.cross_rule = None       # the conflict rule of the redesign: cross_dimer.LengthRule or cross_duplex.DgRule
        self.cross_dimer_rounds = 8
        self.last_cross_rounds = []
        self.last_cross_banned = []
        self.last_cross_dropped = []
        self.last_cross_kept = []

    def _set_either_strand(self, either_strand):
        """Whether a candidate covers a locus whichever strand of it was
        deposited (not an argument of the reference's class): its cover set is
        then rows(scan of s) | rows(scan of revcomp(s)), both scans against the
        targets as given and under the filter's own hybridization model and
        cover extension (_scan_group).  The fixed probes and prune_probe_strs
        get the same.  The picks are the candidates as handed in; of two
        candidates that are each other's reverse complement the first one wins
        the tie and the other then gains nothing."""
        if not isinstance(either_strand, (bool, np.bool_)):
            raise ValueError("either_strand must be True or False, not %r" % (either_strand,))
        self.either_strand = bool(either_strand)

    def _set_target_regions(self, target_regions):
        """The bases that are to be covered at all (not an argument of the
        reference's class): a catch_amd.target_regions.TargetRegions, or its
        per_group value -- per group, per genome, an array of (seq_index, start,
        end) in normal form.  After every scan the cover rows (the fixed probes'
        too) are cut to their runs of wanted bases (engine.Rows.restrict);
        everything behind the scan then works on wanted bases only.
        last_wanted_bases[group] = the group's wanted bases,
        last_coverable_bases[group] = those a candidate's cover range holds."""
        if target_regions is not None and not hasattr(target_regions, "genome_intervals"):
            from catch_amd.target_regions import TargetRegions
            target_regions = TargetRegions(target_regions)
        self.target_regions = target_regions

    def _set_budget(self, max_probes, pick_gains, curve_points):
        """The probe budget and what it rests on (not arguments of the
        reference's class).  pick_gains: after the solve (and the pruning) of a
        group, last_pick_gains[group][i] = the bases its i-th pick covered first
        and last_coverage_curve[group] = rows (k, covered, coverable, worst
        universe, its covered, its denominator) at about curve_points pick
        counts k, the last one included.  max_probes = N (implies pick_gains):
        over all groups only the N picks that a merge of the groups' pick
        sequences by gain takes first are kept (allocate_budget); a probe picked
        for several groups counts once, as the designer writes it once; every group
        keeps a prefix of its picks, last_budget_kept[group] its length.  Only
        at coverage 1.0 without ranks is that the greedy for maximum coverage
        over all groups together."""
        if max_probes is not None:
            if (isinstance(max_probes, bool) or not isinstance(max_probes, (int, np.integer))
                    or max_probes < 1):
                raise ValueError("max_probes must be an integer >= 1 (or None), not %r" % (max_probes,))
            max_probes = int(max_probes)
        if not isinstance(pick_gains, (bool, np.bool_)):
            raise ValueError("pick_gains must be True or False, not %r" % (pick_gains,))
        if (isinstance(curve_points, bool) or not isinstance(curve_points, (int, np.integer))
                or curve_points < 1):
            raise ValueError("curve_points must be an integer >= 1, not %r" % (curve_points,))
        self.max_probes = max_probes
        self.pick_gains = bool(pick_gains) or max_probes is not None
        self.curve_points = int(curve_points)
        if self.pick_gains and self.coverage_depth > 1:
            raise NotImplementedError(
                "pick_gains / max_probes cannot be combined with coverage_depth > 1: "
                "a gain is then no longer the bases covered first")

    def _set_cross_dimer(self, max_cross_dimer, cross_dimer_rounds, max_cross_dimer_dg=None):
        """The cross-dimer redesign (not an argument of the reference's class):
        with max_cross_dimer = X >= 1 no two selected probes, of any group, and
        no selected probe and fixed probe pair with each other over more than X
        bases (catch_amd/filter/cross_dimer.py: conflicts_with) -- or, with
        max_cross_dimer_dg = G in its place, none form a stretch firmer than G
        kcal/mol (catch_amd/filter/cross_duplex.py) -- and what a
        conflicting pick would have covered is covered again by other
        candidates, in at most cross_dimer_rounds = R >= 1 solves per group
        (_cross_rounds has the definition).  last_cross_rounds[group] = the
        solves it took, last_cross_banned[group] = the candidates that were
        never offered to a solve because they conflict with a kept probe or a
        fixed one, last_cross_dropped[group] = the picks dropped,
        last_cross_kept[group] = the probes selected."""
        self.max_cross_dimer = self.max_cross_dimer_dg = self.cross_rule = None
        if max_cross_dimer is None and max_cross_dimer_dg is None:
            return
        from catch_amd.filter import cross_dimer
        rule = cross_dimer.rule_of(max_cross_dimer, max_cross_dimer_dg)
        if (isinstance(cross_dimer_rounds, bool) or not isinstance(cross_dimer_rounds, (int, np.integer))
                or cross_dimer_rounds < 1):
            raise ValueError("cross_dimer_rounds must be an integer >= 1, not %r" % (cross_dimer_rounds,))
        if self.coverage_depth > 1 or self.prune_redundant or self.pick_gains:
            raise NotImplementedError(
                "max_cross_dimer / max_cross_dimer_dg (the cross-dimer redesign) cannot be combined with coverage_depth > 1, "
                "prune_redundant, pick_gains or max_probes")
        self.cross_rule = rule
        self.max_cross_dimer = rule.above if max_cross_dimer_dg is None else None
        self.max_cross_dimer_dg = max_cross_dimer_dg
        self.cross_dimer_rounds = int(cross_dimer_rounds)

    def _set_prune_redundant(self, prune_redundant):
        """Whether the picks are looked at again once the design is complete (not
        an argument of the reference's class): from the last pick to the first,
        one is dropped when every base it covers is covered more than
        coverage_depth times without it (by the other picks and the fixed
        probes).  The bases covered stay the same; last_pruned[group] holds the
        dropped candidates in the order they were dropped."""
        if not isinstance(prune_redundant, (bool, np.bool_)):
            raise ValueError("prune_redundant must be True or False, not %r" % (prune_redundant,))
        self.prune_redundant = bool(prune_redundant)

    def _set_coverage_depth(self, coverage_depth):
        """How many selected probes are to cover every base (not an argument of
        the reference's class): 1 is the reference's set cover, more runs one
        greedy layer per unit of depth (_filter_strs_keeping_rows)."""
        if (isinstance(coverage_depth, bool) or not isinstance(coverage_depth, (int, np.integer))
                or coverage_depth < 1):
            raise ValueError("coverage_depth must be an integer >= 1, not %r" % (coverage_depth,))
        if coverage_depth > 1 and self.fixed_probes:
            raise NotImplementedError(
                "coverage_depth > 1 cannot be combined with fixed_probes")
        self.coverage_depth = int(coverage_depth)

    # ------------------------------------------------------------------
    def _context(self):
        return engine.default_context()

    @property
    def needs_rows(self):
        """Whether an option is on that works on a group's cover rows after the
        scan (_filter_strs_keeping_rows): the fused scan-and-solve call and the
        device front end never hand the rows out."""
        return (bool(self.fixed_probes) or self.coverage_depth > 1 or self.prune_redundant or self.pick_gains
                or self.target_regions is not None or self.either_strand or self.cross_rule is not None)

    def _anchor_table(self, strs, assume_unique=False, tolerant=False):
        """probe.anchor_table of `strs` under the strict hybridization model, or
        the tolerant one (the ranks)."""
        mismatches, lcf_thres = ((self.mismatches_tolerant, self.lcf_thres_tolerant) if tolerant
                                 else (self.mismatches, self.lcf_thres))
        return probe.anchor_table(strs, mismatches, lcf_thres, min_k=self.kmer_probe_map_k,
                                  k=self.kmer_probe_map_k, assume_unique=assume_unique)

    def _model_args(self):
        """The hybridization model and scan mode, as the keywords that
        engine.Rows.scan, setcover_filter and setcover_filter_many share."""
        return dict(mismatches=self.mismatches, lcf_thres=self.lcf_thres, island=self.island_of_exact_match,
                    cover_extension=self.cover_extension, mode=self.scan_mode)

    def _open_group(self, ctx, held, strs, genomes, assume_unique=False, table=None, targets=None):
        """(Targets, Probes) of one instance on `ctx`: the anchor table of `strs`
        (or `table`, drawn earlier) and the sequences of `genomes` (or `targets`,
        which stays the caller's).  What is made here is appended to `held`; the
        caller closes it."""
        k, uniq, owner, ep, eo = table if table is not None else self._anchor_table(strs, assume_unique)
        if targets is None:
            targets = engine.Targets(ctx, [g.seqs for g in genomes])
            held.append(targets)
        probes = engine.Probes(ctx, uniq, owner, ep, eo, k)
        held.append(probes)
        return targets, probes

    def _scan_group(self, ctx, held, strs, genomes, assume_unique=False, table=None, targets=None):
        """_open_group and the cover rows of the probes on the targets ->
        (Targets, Probes, Rows), the Rows in `held` too."""
        if self.either_strand and table is None:
            table = self._anchor_table(strs, assume_unique)     # (the call _open_group would make)
        targets, probes = self._open_group(ctx, held, strs, genomes, assume_unique, table, targets)
        rows = engine.Rows.scan(ctx, probes, targets, **self._model_args())
        if self.either_strand:
            rows = self._either_strand_rows(ctx, rows, table, targets)
        held.append(rows)
        return targets, probes, rows

    def _either_strand_rows(self, ctx, rows, table, targets):
        """`rows` (the scan of `table`'s strings on `targets`, just made on
        `ctx`) united, set by set, with the rows of the reverse-complemented
        strings on the same targets; the two inputs are closed.  The anchors of
        the reverse complements are a table of their own (drawn after the
        forward one where anchors are random), the owners stay.  What the three
        calls took is left in self._strand_scan for _add_scan_times."""
        _k, uniq, owner, _ep, _eo = table
        done = dict(phases={name: ctx.kernel_ms(ph) for name, ph in _SCAN_PHASES}, rows=rows.n)
        rc_probes = rc_rows = None
        try:
            rc_uniq = [_reverse_complement(s) for s in uniq]
            rk, _u, _o, rep, reo = self._anchor_table(rc_uniq, assume_unique=True)
            rc_probes = engine.Probes(ctx, rc_uniq, owner, rep, reo, rk)
            rc_rows = engine.Rows.scan(ctx, rc_probes, targets, **self._model_args())
            # (the verify phase lies inside the scan phase)
            done["rc_scan_ms"] = sum(ctx.kernel_ms(ph)[0] for ph in (engine.PHASE_SCAN, engine.PHASE_ROWS))
            done["rows_rc"] = rc_rows.n
            both = rows.union(rc_rows)
            done["union_ms"] = ctx.kernel_ms(engine.PHASE_ROWS)[0]
            done["rows_union"] = both.n
        finally:
            for h in (rc_rows, rc_probes, rows):
                if h is not None:
                    h.close()
        self._strand_scan = done
        return both

    def _add_scan_times(self, timings, ctx, rows, group=None):
        """The device times and the row count of the _scan_group call that made
        `rows` into `timings`.  Under either_strand scan_ms / rows_ms / rows stay
        those of the forward scan, beside them rc_scan_ms, union_ms, rows_rc and
        rows_union; group = (number, of): the group's log line."""
        if not self.either_strand:
            _add_phase_times(timings, ctx, _SCAN_PHASES)
            timings["rows"] += rows.n
            return
        done = self._strand_scan
        for name, (ms, nl) in done["phases"].items():
            timings[name] = timings.get(name, 0.0) + ms
            ln = name.replace("_ms", "_launches")
            timings[ln] = timings.get(ln, 0) + nl
        timings["rows"] += done["rows"]
        for name in ("rc_scan_ms", "union_ms", "rows_rc", "rows_union"):
            timings[name] = timings.get(name, 0) + done[name]
        if group is not None:
            logger.info("Group %d of %d: either strand: %d rows forward, %d reverse, %d in the union",
                        group[0], group[1], done["rows"], done["rows_rc"], done["rows_union"])

    def _scan_ms(self, ctx):
        """Device time of the last _scan_group call on `ctx`, all of it."""
        ms = sum(ctx.kernel_ms(ph)[0] for ph in (engine.PHASE_SCAN, engine.PHASE_ROWS))     # (the verify phase lies inside the scan phase)
        if self.either_strand:
            done = self._strand_scan
            ms = done["phases"]["scan_ms"][0] + done["phases"]["rows_ms"][0] + done["rc_scan_ms"] + done["union_ms"]
        return ms

    def _make_sets(self, candidate_probes, target_genomes, ctx=None,
                   targets=None):
        """Device rows for one group (:359-470).  Returns (rows, owner) where
        rows is an engine.Rows (set ids = indices into candidate_probes)."""
        ctx = ctx or self._context()
        held = []
        try:
            targets, probes = self._open_group(ctx, held, [p.seq_str for p in candidate_probes],
                                               target_genomes, targets=targets)
            return engine.Rows.scan(ctx, probes, targets, **self._model_args())
        finally:
            for h in reversed(held):
                h.close()

    def _tolerant_bp_over(self, ctx, probes_dev, n_uniq, sequences):
        """Sum over `sequences` and their reverse complements of the bp each
        unique probe covers under the tolerant model (:472-529)."""
        bp = np.zeros(max(n_uniq, 1), dtype=np.int64)
        if not sequences:
            return bp
        # one genome per sequence: coverage is merged per sequence anyway
        genomes = []
        for s in sequences:
            genomes.append([s])
            genomes.append([_reverse_complement(s)])
        t = engine.Targets(ctx, genomes)
        try:
            engine.tolerant_bp(ctx, probes_dev, t, self.mismatches_tolerant,
                               self.lcf_thres_tolerant,
                               self.island_of_exact_match_tolerant, bp)
        finally:
            t.close()
        return bp

    def _make_ranks(self, candidate_probes, target_genomes_grouped, ctx=None):
        return self._make_ranks_strs([p.seq_str for p in candidate_probes],
                                     target_genomes_grouped, ctx)

    def _make_ranks_strs(self, strs, target_genomes_grouped, ctx=None):
        """Rank per candidate (:614-735): (0, #groups hit) under --identify,
        (1, avoided bp) for probes that touch an avoided genome, densified."""
        n = len(strs)
        need = self.identify or len(self.avoided_genomes) > 0
        if not need:
            return np.zeros(n, dtype=np.int64)
        ctx = ctx or self._context()
        k, uniq, _owner, ep, eo = self._anchor_table(strs, tolerant=True)
        ident = np.arange(len(uniq), dtype=np.int32)
        pd = engine.Probes(ctx, uniq, ident, ep, eo, k)
        try:
            if self.identify:
                hits = np.zeros(len(uniq), dtype=np.int64)
                for genomes in target_genomes_grouped:
                    seqs = [s for g in genomes for s in g.seqs]
                    bp = self._tolerant_bp_over(ctx, pd, len(uniq), seqs)
                    hits += (bp[:len(uniq)] >= 1)
                rank_a = np.zeros(len(uniq), dtype=np.int64)
                rank_b = hits
            else:
                rank_a = np.zeros(len(uniq), dtype=np.int64)
                rank_b = np.zeros(len(uniq), dtype=np.int64)
            total = np.zeros(len(uniq), dtype=np.int64)
            for path in self.avoided_genomes:
                for sequence in seq_io.iterate_fasta(path):
                    total += self._tolerant_bp_over(ctx, pd, len(uniq),
                                                    [sequence])[:len(uniq)]
            avoided = total > 0
            rank_a = np.where(avoided, 1, rank_a)
            rank_b = np.where(avoided, total, rank_b)
        finally:
            pd.close()
        tuples = sorted(set(zip(rank_a.tolist(), rank_b.tolist())))
        tidx = {t: i for i, t in enumerate(tuples)}
        uidx = {s: i for i, s in enumerate(uniq)}
        return np.fromiter(
            (tidx[(int(rank_a[uidx[s]]), int(rank_b[uidx[s]]))] for s in strs),
            dtype=np.int64, count=n)

    def _make_universe_p(self, target_genomes):
        """:761-792."""
        if self.coverage <= 1.0:
            return [self.coverage for _ in target_genomes]
        out = []
        for gnm in target_genomes:
            desired = min(self.coverage, gnm.size())
            out.append(float(desired) / gnm.size())
        return out

    def _filter(self, input, target_genomes_grouped):
        """input = [p_1, ..., p_m] candidate probes per group; returns the
        selected probes per group (:902-930)."""
        input = [list(pp) for pp in input]
        ids = self._filter_strs([[p.seq_str for p in pp] for pp in input],
                                target_genomes_grouped)
        return [[pp[i] for i in sel] for pp, sel in zip(input, ids)]

    def _filter_strs(self, input_strs, target_genomes_grouped,
                     assume_unique=False, only=None, tables=None):
        """The filter on plain probe strings: per group the indices of the
        selected candidates, in pick order.  Groups are independent instances:
        up to CATCHHIP_GROUPS_IN_FLIGHT (default 4) of them run at once, each
        on its own context / HIP stream (catchhip_setcover_filter_many).
        assume_unique: the strings of a group are pairwise distinct (they come
        out of the duplicate filter).  only: restrict the work to these group
        indices (the others come back empty; multi-rank runs).  With more than
        one rank (catch_amd.parallel.init_from_env) the groups are spread over
        the ranks and every rank returns the complete selection."""
        import os
        from catch_amd import parallel
        if self.needs_rows:
            return self._filter_strs_keeping_rows(input_strs, target_genomes_grouped,
                                                  assume_unique)
        if only is None and parallel.world().size > 1:
            return self._filter_strs_multirank(input_strs, target_genomes_grouped,
                                               assume_unique, parallel.world())
        selected = [[] for _ in input_strs]
        timings = _new_timings()
        nonempty = [i for i, pp in enumerate(input_strs) if len(pp) > 0]
        todo = [i for i in nonempty if only is None or i in only]
        random_anchors = any(probe.anchors_use_random(
            input_strs[i], self.mismatches, self.lcf_thres, self.kmer_probe_map_k)
            for i in nonempty)
        width = max(1, int(os.environ.get("CATCHHIP_GROUPS_IN_FLIGHT", "4")))
        # many SMALL groups go through one instance (its anchors are the groups'
        # anchors drawn back to back, in input order); large groups (thousands of
        # candidates each) overlap better as separate instances in flight
        if (only is None and tables is None
                and assume_unique and not self.identify and not self.avoided_genomes
                and len(todo) >= int(_lib.test_env("CATCHHIP_UNION_MIN_GROUPS", "8"))
                and sum(len(input_strs[gi]) for gi in todo) <= len(todo) * 8192
                and len({len(s) for gi in todo for s in input_strs[gi]}) == 1):
            self._filter_strs_union(input_strs, target_genomes_grouped, todo,
                                    selected, timings)
            todo = []
        # Random anchors (catch/probe.py:391-401) consume np.random once per
        # probe, group after group in INPUT order, while the groups below run
        # largest first (and, over several ranks, only some of them here): the
        # tables of all groups are then drawn up front, in input order, so that
        # every schedule selects what the reference selects.
        # (With --identify / --avoid-genomes the rank tables draw too, interleaved
        # with the set tables group by group: then the groups simply keep their
        # input order.)
        need_ranks = self.identify or len(self.avoided_genomes) > 0
        in_input_order = random_anchors and need_ranks and tables is None
        if todo and random_anchors and tables is None and not need_ranks:
            tables = self._anchor_tables_in_input_order(input_strs, nonempty,
                                                        assume_unique)
        if in_input_order:
            chunks = [todo[i:i + width] for i in range(0, len(todo), width)]
        else:
            # largest first, as the reference hands its instances to the pool
            # (catch/filter/set_cover_filter.py:880-887)
            todo.sort(key=lambda i: (-len(input_strs[i]), i))
            chunks = _chunks_by_size(
                todo, lambda gi: sum(g.size() for g in target_genomes_grouped[gi]), width)
        for chunk in chunks:
            ctxs = _contexts(len(chunk))
            specs, held, all_ranks = [], [], []
            try:
                for ctx, gi in zip(ctxs, chunk):
                    strs, target_genomes = \
                        input_strs[gi], target_genomes_grouped[gi]
                    logger.info("Building set cover sets input (group %d of %d)",
                                gi + 1, len(input_strs))
                    targets, probes = self._open_group(
                        ctx, held, strs, target_genomes, assume_unique,
                        table=tables.pop(gi) if tables is not None else None)
                    ranks = self._make_ranks_strs(strs, target_genomes_grouped,
                                                  ctx)
                    all_ranks.append(ranks)
                    specs.append((ctx, probes, targets, len(strs),
                                  ranks if ranks.any() else None,
                                  self._make_universe_p(target_genomes)))
                logger.info("Solving set cover instances (groups %s of %d)",
                            [gi + 1 for gi in chunk], len(input_strs))
                results = engine.setcover_filter_many(specs, **self._model_args())
            finally:
                for h in held:
                    h.close()
            for ctx, gi, ranks, (ids, nrows) in zip(ctxs, chunk, all_ranks,
                                                    results):
                _accumulate(timings, ctx, nrows, len(ids))
                _warn_less_than_ideal(gi, ranks, ids)
                selected[gi] = list(ids)
        self.last_timings = timings
        return selected

    def _filter_strs_keeping_rows(self, input_strs, target_genomes_grouped,
                                  assume_unique=False):
        """_filter_strs for the options that work on a group's cover rows
        (needs_rows): one group after the other on one context, in input order,
        one scan of the candidates per group.  Per group:

        1. The scan -> `rows`.
           Under either_strand it is the union of two scans, the candidates'
           and their reverse complements' (_scan_group), and so is the fixed
           probes' table below.
        2. The first table.  With fixed probes they count as sets picked before
           the first round of the greedy loop (catch/utils/set_cover.py:362-550):
           their coverage C0_u (one more scan; the filter's own hybridization
           model, strands as given) leaves every universe and every candidate's
           rows (Rows.subtract), and as many bases may stay uncovered as in U_u =
           (union of the candidates' rows) + C0_u (extension_fraction).  Without
           them the first table is `rows` under the user's fractions.
        3. coverage_depth = D layers, depth(b) = the number of candidates picked
           so far with a cover row over base b.  Layer 1 solves the first table.
           Layer k > 1 is the rows of the unpicked candidates cut into their runs
           of bases with depth < k (Rows.below_depth); its universe u is those
           n2[u] bases together with the reached[u] bases at depth >= k, of which
           int(|U| - p |U|) may stay below k (extension_fraction restates p for
           the n2[u] bases the solver sees).  The solvers run unchanged, with the
           same ranks in every layer; the first k layers are the design at depth
           k.  A layer with no row left is empty and logged.  (The constructor
           refuses D > 1 with fixed probes: with them this is one layer.)
        4. prune_redundant: the picks of all layers go through Rows.prune at
           depth D, beside the fixed probes' rows, which stay whatever happens
           (the nesting of the layers is lost: a pick of layer 1 may be dropped
           for picks of layer 2); last_layer_sizes stays what the layers picked,
           last_pruned[group] the dropped ones.
        5. pick_gains / max_probes: _Budget, on the first table -- the one that
           went to the solver --, beside it the bases the fixed probes cover.

        The fixed probes' anchors are drawn first, once.  What a run with fixed
        probes reports (last_timings' keys, last_layer_sizes, log lines) differs
        from one without in ways its callers rely on and no stage requires: the
        comments marked (quirk)."""
        from catch_amd import parallel
        fixed = bool(self.fixed_probes)
        regions = self.target_regions
        if parallel.world().size > 1:
            raise NotImplementedError(
                "fixed probes (extending an existing probe set) run on one rank" if fixed else
                "target regions run on one rank" if regions is not None else
                "either_strand runs on one rank" if self.either_strand else
                "the cross-dimer redesign (max_cross_dimer) runs on one rank" if self.cross_rule is not None else
                "coverage_depth > 1, prune_redundant, pick_gains and max_probes run on one rank")
        ctx = self._context()
        ngroups = len(input_strs)
        selected = [[] for _ in input_strs]
        self.last_pruned = [[] for _ in input_strs]
        # (quirk) an extension reports its one layer only when it prunes, and leaves last_layer_sizes alone otherwise
        keeps_sizes = not fixed or self.prune_redundant
        if keeps_sizes:
            self.last_layer_sizes = [[] for _ in input_strs]
        # (quirk) depth_ms only without fixed probes -- depth_launches only once a layer above 1 ran --, and rows_reduced
        # counts the rows of the reduced table with them, of the layers above 1 without
        timings = _new_timings(rows_reduced=0, **(dict(fixed_scan_ms=0.0, subtract_ms=0.0, rows_fixed=0) if fixed
                                                  else dict(depth_ms=0.0)))
        if self.prune_redundant:
            timings.update(prune_ms=0.0, prune_launches=0, prune_rounds=0, pruned=0)
        if self.either_strand:
            timings.update(rc_scan_ms=0.0, union_ms=0.0, rows_rc=0, rows_union=0)
        if regions is not None:
            timings.update(mask_ms=0.0, restrict_ms=0.0, rows_restricted=0)
            self.last_wanted_bases = [0] * ngroups
            self.last_coverable_bases = [0] * ngroups
        budget = _Budget(self, ctx, ngroups, timings)
        redesign = self.cross_rule is not None
        if redesign:
            timings.update(ban_ms=0.0, ban_pairs=0, cross_rounds=0)
            self.last_cross_rounds = [0] * ngroups
            self.last_cross_banned = [0] * ngroups
            self.last_cross_dropped = [0] * ngroups
            self.last_cross_kept = [0] * ngroups
            cross_kept = []          # K: the distinct strings kept so far, over all groups
        if fixed:
            fk, funiq, _fowner, fep, feo = self._anchor_table(self.fixed_probes)
            fixed_table = (fk, funiq, np.zeros(len(funiq), dtype=np.int32), fep, feo)    # one set: only their union matters
        try:
            for gi, strs in enumerate(input_strs):
                if len(strs) == 0:
                    continue
                target_genomes = target_genomes_grouped[gi]
                ng = len(target_genomes)
                if fixed:
                    logger.info("Building set cover sets input (group %d of %d), %d fixed probes",
                                gi + 1, ngroups, len(funiq))
                else:
                    logger.info("Building set cover sets input (group %d of %d), coverage depth %d",
                                gi + 1, ngroups, self.coverage_depth)
                held = []
                try:
                    targets, _probes, rows = self._scan_group(ctx, held, strs, target_genomes, assume_unique)
                    self._add_scan_times(timings, ctx, rows, (gi + 1, ngroups))
                    p = self._make_universe_p(target_genomes)
                    mask = None
                    if regions is not None:
                        # the rows cut to the wanted bases: from here on the universes, the gains, the depth and the
                        # redundancy are those of wanted bases
                        mask = engine.BaseMask(ctx, [sum(len(s) for s in g.seqs) for g in target_genomes],
                                               *regions.genome_intervals(gi, target_genomes))
                        held.append(mask)
                        timings["mask_ms"] += mask.last_build_ms
                        self.last_wanted_bases[gi] = int(mask.wanted.sum())
                        rows = self._restrict_rows(ctx, held, rows, mask, timings)
                        timings["rows_restricted"] += rows.n
                        coverable = rows.stats(ng)[1]
                        self.last_coverable_bases[gi] = int(coverable.sum())
                        if self.last_wanted_bases[gi] == 0:
                            logger.warning("Group %d of %d: the target regions leave no base to cover; "
                                           "no probe is selected for it", gi + 1, ngroups)
                            continue
                        if self.coverage > 1:       # a number of bases: of the wanted bases a candidate can cover
                            p = [_bases_fraction(int(n), self.coverage) for n in coverable]
                    if fixed:
                        frows = self._scan_group(ctx, held, None, None, table=fixed_table, targets=targets)[2]
                        timings["fixed_scan_ms"] += self._scan_ms(ctx)
                        if mask is not None:
                            frows = self._restrict_rows(ctx, held, frows, mask, timings)
                        first = rows.subtract(frows)
                        held.append(first)
                        timings["subtract_ms"] += ctx.kernel_ms(engine.PHASE_ROWS)[0]
                        timings["rows_fixed"] += frows.n
                        timings["rows_reduced"] += first.n
                        n2, covered0 = first.stats(ng)[1], frows.stats(ng)[1]
                        first_p = [extension_fraction(int(a), int(b), q) for a, b, q in zip(n2, covered0, p)]
                        denom = n2 + covered0
                    else:
                        frows, first, first_p, covered0 = None, rows, p, None
                    ranks = self._make_ranks_strs(strs, target_genomes_grouped, ctx)
                    rk = ranks if ranks.any() else None
                    ids, sizes = [], []
                    if redesign:
                        # (target regions at a coverage above 1: p counts the bases the OFFERED candidates can cover)
                        ids = self._cross_rounds(ctx, gi, ngroups, strs, first, p, covered0, rk, ng, cross_kept, timings,
                                                 coverable_of=rows if mask is not None and self.coverage > 1 else None)
                        sizes = [len(ids)]
                    for layer in range(1, 1 if redesign else self.coverage_depth + 1):
                        if layer == 1:
                            table, universe_p = first, first_p
                        else:
                            table, reached = rows.below_depth(len(strs), ids, layer)
                            held.append(table)
                            _add_phase_times(timings, ctx, (("depth_ms", engine.PHASE_ROWS),))
                            timings["rows_reduced"] += table.n
                            if table.n == 0:
                                # (not the end: a base that `layer` picks hold lies below the next layer's depth)
                                logger.info("Group %d of %d: no candidate is left to raise any base to "
                                            "depth %d; layer %d is empty", gi + 1, ngroups, layer, layer)
                                held.remove(table)
                                table.close()
                                sizes.append(0)
                                continue
                            universe_p = [extension_fraction(int(a), int(b), q)
                                          for a, b, q in zip(table.stats(ng)[1], reached, p)]
                        if fixed:
                            logger.info("Solving the set cover instance of group %d of %d", gi + 1, ngroups)
                        else:
                            logger.info("Solving the set cover instance of group %d of %d, layer %d of %d",
                                        gi + 1, ngroups, layer, self.coverage_depth)
                        got = table.greedy(len(strs), rk, _solver_fractions(universe_p))
                        _add_phase_times(timings, ctx, _GREEDY_PHASES)
                        if layer > 1:
                            held.remove(table)
                            table.close()
                        ids += got
                        sizes.append(len(got))
                    if self.prune_redundant:
                        ids, self.last_pruned[gi] = _prune(ctx, rows, len(strs), ids, self.coverage_depth, frows,
                                                           timings)
                    timings["picks"] += len(ids)
                    if self.pick_gains:
                        budget.group(gi, first, len(strs), ids, denom if fixed else rows.stats(ng)[1], covered0)
                finally:
                    for h in reversed(held):
                        if not budget.holds(h):
                            h.close()
                if not fixed:       # (quirk) an extension logs neither line
                    logger.info("Group %d of %d: picks per layer %s", gi + 1, ngroups,
                                " / ".join(str(x) for x in sizes))
                    if self.prune_redundant:
                        logger.info("Group %d of %d: %d picked, %d redundant", gi + 1, ngroups,
                                    sum(sizes), len(self.last_pruned[gi]))
                _warn_less_than_ideal(gi, ranks, ids)
                selected[gi] = list(ids)
                if keeps_sizes:
                    self.last_layer_sizes[gi] = sizes
            budget.finish(selected, input_strs)
        finally:
            budget.release()         # (a group that raised: the tables kept for the cut)
        self.last_timings = timings
        return selected

    @staticmethod
    def _restrict_rows(ctx, held, rows, mask, timings):
        """`rows` (in `held`) replaced by its cut to the wanted bases of `mask`:
        the whole table goes back to the pool at once."""
        cut = rows.restrict(mask)
        held.append(cut)
        timings["restrict_ms"] += ctx.kernel_ms(engine.PHASE_ROWS)[0]
        held.remove(rows)
        rows.close()
        return cut

    def _cross_rounds(self, ctx, gi, ngroups, strs, first, p, covered0, rk, ng, kept_all, timings, coverable_of=None):
        """The repair rounds of one group under max_cross_dimer = X and
        cross_dimer_rounds = R -> the group's selection, in the order kept.
        Under max_cross_dimer_dg = G the loop is the same and `conflicts` reads
        duplex > floor(100 G) for run > X: the bans and the pick walk come from
        the rule in force (self.cross_rule).

        E = the fixed probes' strings, K = `kept_all`, the distinct strings kept
        so far over all groups (extended here), K_g its part kept for this
        group, C_g = `strs`.  For round r = 0, 1, ...:

          A_r     = the candidates of C_g, in order, that are not in K_g and do
                    not conflict with a record of E ++ K (conflicts_with).
          picks_r = what SetCoverFilter(the same model, fixed_probes=E ++ K_g)
                    selects for the one group A_r, in pick order; with E and K_g
                    empty that is the plain filter.
          the walk: a pick is kept iff no pick kept earlier in THIS walk
                    conflicts with it (none can conflict with E ++ K); the kept
                    ones join K_g, and K unless already there.  A dropped pick
                    conflicts with a member of K now and is never offered again.
          the end:  picks_r is empty, or nothing was dropped, or r = R - 1 --
                    then with a warning if the last walk dropped something.

        So: no two probes of the output conflict and none conflicts with E.  With
        X at or above the longest candidate nothing is banned or dropped and the
        result is the plain design's.  Round 0 of a group with nothing banned
        and nothing dropped IS the filter without the option: K of other groups
        never counts as cover, only as a source of bans.  Every continuing round
        drops a pick for good, so the loop ends without the cap, which bounds
        time only.  A kept probe c with run(c, c) > X bans its own copies in
        later groups (max_self_dimer in front removes such candidates); equal
        strings are not exempted.

        One scan per group: round r's table is derived on the device from
        `first` (the group's rows, minus the fixed probes' when there are any):
        Rows.below_depth(K_g's ids, 1) takes the kept picks out, cuts what they
        cover and counts it (`reached`, which joins the fixed probes' covered0 in
        extension_fraction), Rows.drop_sets takes the banned candidates out.
        Set ids stay C_g's, so ties fall as they do among A_r.  The bans are
        engine.cross_against_flags of C_g against what joined E ++ K since the
        last look; the walk is the conflict graph's naive() -- both on the host
        path (cross_dimer.cross_against_numpy, walk) under
        CATCHHIP_HOST_FRONT_END=1 or with a record of more than 256 characters."""
        from catch_amd.filter import cross_dimer
        rule, R = self.cross_rule, self.cross_dimer_rounds
        n = len(strs)
        on_host = cross_dimer._on_host(list(strs) + self.fixed_probes + kept_all)
        index_of = {}
        for i, s in enumerate(strs):
            index_of.setdefault(s, []).append(i)
        known = set(kept_all)
        banned = np.zeros(n, dtype=bool)
        in_kg = np.zeros(n, dtype=bool)
        kg_ids = []                      # every index of C_g that holds a string of K_g (equal strings: equal rows)
        selected = []
        pending = self.fixed_probes + kept_all      # what C_g has not been held against yet
        base0 = np.zeros(ng, dtype=np.int64) if covered0 is None else np.asarray(covered0, dtype=np.int64)
        rounds = dropped = 0
        while True:
            if pending:
                if on_host:
                    banned |= rule.flags_host(strs, pending)
                else:
                    banned |= rule.flags_device(ctx, strs, pending)
                    timings["ban_ms"] += ctx.kernel_ms(engine.PHASE_NDF)[0]
                timings["ban_pairs"] += n * len(pending)
            offered_out = banned & ~in_kg
            held = []
            try:
                table, reached = first, None
                if kg_ids:
                    table, reached = table.below_depth(n, kg_ids, 1)
                    held.append(table)
                if offered_out.any():
                    table = table.drop_sets(n, offered_out)
                    held.append(table)
                q = p
                if coverable_of is not None:
                    left = coverable_of.drop_sets(n, banned | in_kg)
                    held.append(left)
                    q = [_bases_fraction(int(m), self.coverage) for m in left.stats(ng)[1]]
                if reached is None and covered0 is None:
                    universe_p = q       # (nothing is fixed and nothing kept: the plain instance)
                else:
                    c0 = base0 + (0 if reached is None else reached)
                    universe_p = [extension_fraction(int(a), int(b), f) for a, b, f in zip(table.stats(ng)[1], c0, q)]
                logger.info("Solving the set cover instance of group %d of %d, cross-dimer round %d",
                            gi + 1, ngroups, rounds + 1)
                picks = table.greedy(n, rk, _solver_fractions(universe_p)) if table.n else []
                if table.n:
                    _add_phase_times(timings, ctx, _GREEDY_PHASES)
            finally:
                for h in reversed(held):
                    h.close()
            rounds += 1
            pick_strs = [strs[i] for i in picks]
            if len(picks) < 2:
                keep = np.ones(len(picks), dtype=bool)
            elif on_host:
                keep = rule.walk(pick_strs)
            else:
                graph = rule.graph(ctx, pick_strs)
                try:
                    keep = graph.naive()
                finally:
                    graph.close()
            pending = []
            for i, s, k in zip(picks, pick_strs, keep):
                if not k or in_kg[i]:    # (dropped, or an equal string was kept a moment ago: K_g holds distinct strings)
                    continue
                selected.append(i)
                for j in index_of[s]:
                    in_kg[j] = True
                    kg_ids.append(j)
                if s not in known:
                    known.add(s)
                    kept_all.append(s)
                    pending.append(s)
            ndrop = len(picks) - int(np.count_nonzero(keep))
            dropped += ndrop
            if not picks or ndrop == 0:
                break
            if rounds == R:
                logger.warning("group %d: round cap %d reached, %d picks dropped without a redesign", gi + 1, R, ndrop)
                break
        timings["cross_rounds"] += rounds
        self.last_cross_rounds[gi] = rounds
        self.last_cross_banned[gi] = int(np.count_nonzero(banned & ~in_kg))
        self.last_cross_dropped[gi] = dropped
        self.last_cross_kept[gi] = len(selected)
        return selected

    def prune_probe_strs(self, probe_strs, target_genomes):
        """Which probes of an existing list can go without uncovering a base?
        Every string is a set of its own (equal strings too) and every one is
        picked, in the order given; one scan against `target_genomes` (one
        universe each) under this filter's hybridization model and cover
        extension, then Rows.prune at coverage_depth.  Returns (indices kept, in
        the order given; indices dropped, last examined last): the last strings
        are examined first.  `coverage` plays no part: no base that the list
        covers coverage_depth times (or as often as it can) is lost."""
        from catch_amd import parallel
        if parallel.world().size > 1:
            raise NotImplementedError("pruning a probe list runs on one rank")
        probe_strs = list(probe_strs)
        timings = dict(scan_ms=0.0, rows_ms=0.0, rows=0, picks=0, prune_ms=0.0,
                       prune_launches=0, prune_rounds=0, pruned=0)
        if not probe_strs:
            self.last_timings = timings
            return [], []
        ctx = self._context()
        held = []
        try:
            rows = self._scan_group(ctx, held, probe_strs, target_genomes, assume_unique=True)[2]
            if self.either_strand:
                self._add_scan_times(timings, ctx, rows)
            else:
                timings["scan_ms"] = ctx.kernel_ms(engine.PHASE_SCAN)[0]
                timings["rows_ms"] = ctx.kernel_ms(engine.PHASE_ROWS)[0]
                timings["rows"] = rows.n
            kept, removed = _prune(ctx, rows, len(probe_strs), list(range(len(probe_strs))),
                                   self.coverage_depth, None, timings)
            timings["picks"] = len(kept)
        finally:
            for h in reversed(held):
                h.close()
        self.last_timings = timings
        return kept, removed

    def _anchor_tables_in_input_order(self, input_strs, nonempty, assume_unique):
        """{group: anchor table} for all non-empty groups, drawn in input order,
        when the anchors are random; None when they are the pigeonhole anchors
        (no random numbers: tables are then built where they are used)."""
        if not any(probe.anchors_use_random(input_strs[i], self.mismatches,
                                            self.lcf_thres, self.kmer_probe_map_k)
                   for i in nonempty):
            return None
        return {i: self._anchor_table(input_strs[i], assume_unique) for i in nonempty}

    def _filter_strs_multirank(self, input_strs, target_genomes_grouped,
                               assume_unique, W):
        """The filter over W.size ranks (one process per GPU).  Level 1: whole
        groups go to ranks longest first (the reference's pool order,
        catch/filter/set_cover_filter.py:880-887), no collective.  Level 2: a
        group above an even share of the bases is sharded over ALL ranks by
        universes: every rank scans the group's candidates against its own
        range of genomes and the frontier solver's rounds exchange the
        per-candidate gains (RCCL all-reduce, catch_amd/parallel.py).  Ranks
        (identify / avoided genomes) are computed by every rank for the groups
        it shares.  Every rank returns every group's selection."""
        import os
        from catch_amd import parallel
        n = len(input_strs)
        if ((self.identify or self.avoided_genomes) and any(
                probe.anchors_use_random(input_strs[i], self.mismatches, self.lcf_thres,
                                         self.kmer_probe_map_k) for i in range(n))):
            # random anchors for the set AND the rank tables, interleaved group by
            # group: every rank does every group, in input order
            return self._filter_strs(input_strs, target_genomes_grouped, assume_unique,
                                     only=set(range(n)))
        costs = [sum(g.size() for g in target_genomes_grouped[i]) if len(input_strs[i]) else 0
                 for i in range(n)]
        # (ranks -- identify / avoided genomes -- and partial coverage are sharded too since round 4: every rank computes
        # the group's ranks itself, they only gate which sets may claim; need[u] and the acceptance thresholds of a
        # universe live on the rank that owns it, the candidates' verdicts travel with the lost marks)
        eligible = True
        # (a group with fewer genomes than ranks is not sharded: some rank would hold an empty shard)
        sharded, whole = parallel.plan_with_sharding(
            costs, W.size,
            min_cost=int(os.environ.get("CATCHHIP_SHARD_MIN_BASES", "30000000"))
            if eligible else float("inf"),
            eligible=[len(target_genomes_grouped[i]) >= W.size for i in range(n)])
        selected = [[] for _ in range(n)]
        timings = _new_timings(sharded_groups=list(sharded))
        ctx = W.comm_ctx
        fallback = []
        nonempty = [i for i in range(n) if len(input_strs[i]) > 0]
        # Random anchors: every rank must scan a sharded group with the SAME tables, and the
        # selection must be the single-rank one: rank 0's np.random state goes to every rank before
        # the tables of all groups are drawn (in input order, as one rank draws them)
        if any(probe.anchors_use_random(input_strs[i], self.mismatches, self.lcf_thres,
                                        self.kmer_probe_map_k) for i in nonempty):
            np.random.set_state(W.broadcast(np.random.get_state()))
        tables = self._anchor_tables_in_input_order(input_strs, nonempty, assume_unique)
        for gi in sharded:                       # all ranks together, same order
            strs, genomes = input_strs[gi], target_genomes_grouped[gi]
            logger.info("Set cover of group %d of %d sharded over %d ranks",
                        gi + 1, n, W.size)
            rows = shard = None
            held = []
            err, qualifies = None, False
            try:
                # a failure on one rank (out of memory, a library error) is reported to ALL ranks below:
                # nobody may walk into the solver's all-reduces alone
                try:
                    b = parallel.split_universes([g.size() for g in genomes], W.size)
                    rows = self._scan_group(ctx, held, strs, genomes[b[W.rank]:b[W.rank + 1]], assume_unique,
                                            table=tables[gi] if tables is not None else None)[2]
                    ranks = (self._make_ranks_strs(strs, target_genomes_grouped, ctx)
                             if (self.identify or self.avoided_genomes) else None)
                    try:
                        up_all = self._make_universe_p(genomes)
                        part = any(p_ < 1.0 for p_ in up_all)     # (the same on every rank)
                        # partial-ness is a property of the INSTANCE: a rank whose own genomes all have p == 1
                        # (coverage in bases, genomes shorter than it) still builds a partial shard -- the same
                        # kernels, round shape and refusals on every rank
                        shard = engine.Shard(rows, len(strs), ranks,
                                             up_all[b[W.rank]:b[W.rank + 1]] if part else None,
                                             instance_partial=part)
                        held.append(shard)
                        qualifies = True
                    except ValueError as exc:
                        # the expected refusal: rows too long or too many sets for the sharded kernels -> whole group
                        if "solved unsharded" not in str(exc):
                            raise
                except Exception as exc:          # noqa: BLE001 -- reported collectively
                    err = "%s: %s" % (type(exc).__name__, exc)
                status = W.allgather((err, qualifies))
                W_errs = [(r, e) for r, (e, _q) in enumerate(status) if e]
                if W_errs:
                    raise RuntimeError("sharded set cover of group %d failed: %s" % (
                        gi + 1, "; ".join("rank %d: %s" % re for re in W_errs)))
                # every rank must take the same path
                if all(q for _e, q in status):
                    selected[gi] = parallel.sharded_solve([shard], W.exchange_for([shard]), W.native_for([shard]))
                    timings["rows"] += rows.n
                    timings["picks"] += len(selected[gi])
                else:
                    fallback.append(gi)
            finally:
                for h in reversed(held):
                    h.close()
        # groups that could not be sharded after all go whole to the least loaded rank
        loads = [sum(costs[i] for i in w) for w in whole]
        for gi in fallback:
            r = min(range(W.size), key=lambda q: (loads[q], q))
            whole[r].append(gi)
            loads[r] += costs[gi]
        err, mine = None, None
        try:
            mine = self._filter_strs(input_strs, target_genomes_grouped, assume_unique,
                                     only=set(whole[W.rank]), tables=tables)
        except Exception as exc:                  # noqa: BLE001 -- reported collectively
            err = "%s: %s" % (type(exc).__name__, exc)
        W.agree(err)                              # a rank that failed must not leave the others in the gather
        for k_, v in self.last_timings.items():
            if isinstance(v, (int, float)):
                timings[k_] = timings.get(k_, 0) + v
        parts = W.allgather({gi: mine[gi] for gi in whole[W.rank]})
        for part in parts:
            for gi, ids in part.items():
                selected[gi] = ids
        self.last_timings = timings
        return selected

    def _filter_genomes_device(self, target_genomes_grouped, probe_length,
                               probe_stride, seq_length_to_skip=None,
                               near_duplicate_filter=None, return_ids=False,
                               pre_filters=()):
        """[DuplicateFilter | near-duplicate filter, SetCoverFilter] with the
        front end on the device (near_duplicate_filter: an LSH filter object to
        apply to the unique candidates, in their multiplicity order, before the
        set cover):
        per group the candidate windows of its genomes are enumerated and
        de-duplicated on the GPU (catchhip_candidates_create), gathered into a
        probes object and solved; only the selected candidates are looked up
        again, as slices of the host's sequence strings.  Returns the selected
        probe strings per group, in pick order (return_ids: the ids of the
        selected unique candidates instead -- what bench.py's M2 figure times:
        pack + H2D + front end + scan + solve + ids out).  No ranks (identify /
        avoided genomes need every candidate's string)."""
        import os
        assert not self.identify and not self.avoided_genomes
        out = [[] for _ in target_genomes_grouped]
        timings = _new_timings(candidates=0, unique_candidates=0)
        import time as _time
        events, t_call = [], _time.perf_counter()      # (stage, item, start, end): the pipeline's timeline
        todo = [i for i, g in enumerate(target_genomes_grouped) if len(g) > 0]
        width = max(1, int(os.environ.get("CATCHHIP_GROUPS_IN_FLIGHT", "4")))
        sizes = {i: sum(g.size() for g in target_genomes_grouped[i]) for i in todo}
        # largest first (catch/filter/set_cover_filter.py:880-887); the random
        # anchors of a group are drawn when its turn comes, so that order is kept
        # only when no random numbers are involved
        # (nor while an LSH near-duplicate filter draws its positions / hash
        # functions from `random` group after group)
        keep_input_order = not (near_duplicate_filter is None and not probe.anchors_use_random(
            ["A" * probe_length], self.mismatches, self.lcf_thres, self.kmer_probe_map_k))
        # Small groups as ONE instance (as _filter_genomes_device_union does for the clusters of a clustered
        # design): a group of a few Mbases is a chain of ~60 launches that the GPU finishes in microseconds
        # each, and ten such groups one after the other are ten chains -- their union is one (S4 with resident inputs, the 17
        # groups below 32 Mbases: 69.6 -> 60.4 ms; from host strings with three lanes the groups below 16 Mbases:
        # 0.182 -> 0.178 s per pass, while a union of 247 Mbases unbalances the lanes: 0.30 s -- hence the default;
        # every group's picks and their order are its own: test_union_of_groups_equals_per_group).  Only without random numbers in the building of a group
        # (the draws of a union would come in another order than group by group).  An "item" below is a list of
        # group numbers: one group, or the groups of a union.
        union_below = int(float(os.environ.get("CATCHHIP_UNION_SMALL_BELOW_MBASES", "16")) * 1e6)
        items = {}
        if not keep_input_order and union_below > 0:
            small = [i for i in todo if sizes[i] < union_below]
            at = 0
            while len(small) - at >= 2:
                take, b = [], 0
                while at < len(small) and (not take or b + sizes[small[at]] <= 300_000_000):
                    take.append(small[at])
                    b += sizes[small[at]]
                    at += 1
                if len(take) < 2:
                    break
                key = take[0]                         # an item goes by its first group's number
                items[key] = take
                sizes[key] = b
                todo = [i for i in todo if i not in take[1:]]
        for i in todo:
            items.setdefault(i, [i])
        if not keep_input_order:
            todo.sort(key=lambda i: (-sizes[i], i))
            chunks = _chunks_by_size(todo, lambda gi: sizes[gi], width)
        else:
            chunks = [todo[i:i + width] for i in range(0, len(todo), width)]
        # The inputs of the NEXT groups are packed and uploaded while the current
        # chunk is scanned and solved: a helper thread builds (targets, candidates,
        # probes) on the upload context -- host gather into pinned memory, H2D,
        # the front-end kernels on that context's stream -- in the order the
        # chunks consume them (so `random` / np.random are drawn from in the same
        # order as without the overlap), at most CATCHHIP_PREFETCH_DEPTH groups
        # ahead; the finished objects change hands (engine.*.rebind).
        depth = int(os.environ.get("CATCHHIP_PREFETCH_DEPTH", "2"))
        order = [gi for chunk in chunks for gi in chunk]

        def genomes_of(gi):
            return [g for member in items[gi] for g in target_genomes_grouped[member]]

        def universe_p_of(gi):
            return [p for member in items[gi] for p in self._make_universe_p(target_genomes_grouped[member])]

        def build(gi, ctx=None):
            uctx = ctx or engine.upload_context()
            target_genomes = genomes_of(gi)
            made = []
            t_b0 = _time.perf_counter()
            try:
                targets = engine.Targets(uctx, [g.seqs for g in target_genomes])
                made.append(targets)
                events.append(("pack", gi, t_b0 - t_call, _time.perf_counter() - t_call))
                if len(items[gi]) > 1:
                    targets.set_groups(np.repeat(np.arange(len(items[gi])),
                                                 [len(target_genomes_grouped[member]) for member in items[gi]]))
                cands = engine.Candidates(uctx, targets, probe_length,
                                          probe_stride, seq_length_to_skip)
                made.append(cands)
                ncand, nuniq = cands.ncandidates, cands.n
                for f in pre_filters:     # functions of the candidate alone (poly(A)): before the near-duplicate filter
                    f._apply_to_candidates(cands)
                if near_duplicate_filter is not None:
                    if len(items[gi]) > 1:
                        near_duplicate_filter._apply_to_grouped_candidates(cands, len(items[gi]))
                    else:
                        near_duplicate_filter._apply_to_candidates(cands)
                probes = _probes_of_candidates(cands, _anchors_for_candidates(
                    cands.n, probe_length, self.mismatches, self.lcf_thres, self.kmer_probe_map_k))
                made.append(probes)
                events.append(("build", gi, t_b0 - t_call, _time.perf_counter() - t_call))
            except BaseException:
                for h in reversed(made):
                    h.close()
                raise
            return targets, cands, probes, ncand, nuniq

        def discard(res):
            for h in (res[2], res[1], res[0]):
                h.close()

        # Lanes (CATCHHIP_GROUP_LANES=1, the default with the prefetch on): `width` worker threads, each with
        # its own context / stream and a FIXED list of groups (longest-processing-time-first over the
        # groups' sizes, so the same group meets the same context -- and its cached device blocks -- on
        # every call); a lane starts its next group as soon as it is free: the largest group keeps one
        # lane busy while the others work through the rest, instead of chunks that wait for their slowest
        # member.  The groups are still BUILT one at a time by one thread, in an order that serves the
        # lanes as they become free (and, when random numbers are drawn while building, simply in
        # `order`: the draws must stay where they are).
        # (CATCHHIP_GROUP_LANES: 0 = off, chunks instead; 1 = three lanes -- S4 from host strings: 0.187 s per
        # pass with three, 0.192 with four, 0.205 with two, 0.215 in chunks --; n >= 2 = that many)
        lane_env = int(os.environ.get("CATCHHIP_GROUP_LANES", "1"))
        lanes = depth > 0 and lane_env != 0 and len(order) > 1
        lane_count = 3 if lane_env == 1 else lane_env
        pre = feed = None
        # (several devices, CATCHHIP_DEVICES: the chunks' contexts sit on different GPUs and an object built on the one
        # upload context cannot change hands across devices -- every group is then built on its own context)
        if depth > 0 and not lanes and len(set(_devices())) == 1:
            pre = engine.Prefetch(order, build, depth, discard)
            feed = iter(pre)

        def finish(ctx, gi, targets, cands, probes, ncand, nuniq, ids, nrows, lock=None):
            """An item's result into out / timings (lock: several lanes finish groups at once)."""
            members = items[gi]
            target_genomes = genomes_of(gi)
            ids_arr = np.asarray(ids, dtype=np.int64)
            if return_ids:
                res = ids
            else:
                seqs = [s for g in target_genomes for s in g.seqs]
                pos = cands.positions(ids_arr)
                which = np.searchsorted(targets.seq_off, pos, side="right") - 1
                local = pos - targets.seq_off[which]
                res = [seqs[q][o:o + probe_length]
                       for q, o in zip(which.tolist(), local.tolist())]
            if len(members) > 1:
                # a union: every group's own picks, in its own order; ids count from the group's first candidate
                cgrp = cands.groups()
                per_group = np.bincount(cgrp, minlength=len(members))
                first = np.concatenate([[0], np.cumsum(per_group)])
                pick_grp = cgrp[ids_arr] if ids_arr.size else np.zeros(0, dtype=np.int64)
                sel = np.argsort(pick_grp, kind="stable")          # (every group's picks together, in their order)
                g_sorted = pick_grp[sel]
                bounds = np.searchsorted(g_sorted, np.arange(len(members) + 1)).tolist()
                local = (ids_arr[sel] - first[g_sorted]).tolist() if return_ids else [res[q] for q in sel.tolist()]
                parts, units = [], 0.0
                for m, member in enumerate(members):
                    parts.append(local[bounds[m]:bounds[m + 1]])
                    units += float(per_group[m]) * float(sum(g.size() for g in target_genomes_grouped[member]))
            else:
                parts = [res]
                units = float(cands.n) * float(sum(g.size() for g in target_genomes))
            if lock is not None:
                lock.acquire()
            try:
                for member, part in zip(members, parts):
                    out[member] = part
                timings["candidates"] += ncand
                timings["unique_candidates"] += nuniq
                timings["probe_bp_units"] = timings.get("probe_bp_units", 0.0) + units
                _accumulate(timings, ctx, nrows, len(ids))
            finally:
                if lock is not None:
                    lock.release()

        try:
            if lanes:
                import threading
                nl = max(1, min(lane_count, len(order)))
                ctxs = _contexts(nl)
                # What an item costs a lane: its bases plus a fixed share (round 5: a 25-Mbase group takes 7-9 ms, the
                # 265-Mbase one 62 -- ~12 Mbases' worth of launches and read-backs per instance; with plain sizes the
                # lane that got the eight medium groups of S4 ran 40 ms longer than the lane with the large one)
                fixed = float(os.environ.get("CATCHHIP_LANE_FIXED_MBASES", "12")) * 1e6
                cost = {gi: sizes[gi] + fixed for gi in order}
                lists = [[order[j] for j in lane] for lane in _lpt([cost[gi] for gi in order], nl)]
                lane_of = {gi: li for li, lst in enumerate(lists) for gi in lst}
                if keep_input_order:
                    production = list(order)
                else:
                    # the order in which the lanes will ask for their groups if time goes as cost
                    # (round 6, measured and dropped: the lanes' first items produced smallest first, so that the device has
                    # work after a few milliseconds instead of the ~21 ms the largest group takes to pack: 0.1206 vs 0.1220 s)
                    production, at, clock = [], [0] * nl, [0.0] * nl
                    while len(production) < len(order):
                        li = min((l for l in range(nl) if at[l] < len(lists[l])), key=lambda l: (clock[l], l))
                        gi = lists[li][at[li]]
                        production.append(gi)
                        clock[li] += cost[gi]
                        at[li] += 1
                if keep_input_order:
                    # (the lanes then take their groups in production order too)
                    lists = [[gi for gi in production if lane_of[gi] == li] for li in range(nl)]
                cv = threading.Condition()
                built, errors = {}, []
                slots = threading.Semaphore(max(2, depth) * nl)
                res_lock = threading.Lock()

                # ONE builder, which takes the items in production order (so the draws of a build that draws random
                # numbers -- random anchors, a near-duplicate filter -- stay in that order).  Measured in round 5 on S4
                # from host strings: two builders, or lanes balanced by cost instead of size, leave the pass at 0.128-0.133 s
                # -- the three lanes' kernels share one device, and the pass is within ~10 % of the device work it holds
                # (96 ms of scans and solves one chain at a time + ~20 ms of front-end kernels + 0.5 GB of uploads).
                def producer():
                    for gi in production:
                        slots.acquire()
                        if errors:
                            slots.release()
                            return
                        try:
                            # built on the upload context of the DEVICE whose lane will consume it: with CATCHHIP_DEVICES
                            # the lanes sit on several GPUs, and an object cannot change hands across devices
                            res = build(gi, engine.upload_context(ctxs[lane_of[gi]].device))
                        except BaseException as exc:
                            with cv:
                                errors.append(exc)
                                cv.notify_all()
                            return
                        with cv:
                            built[gi] = res
                            cv.notify_all()

                def lane(li):
                    ctx = ctxs[li]
                    for gi in lists[li]:
                        with cv:
                            while gi not in built and not errors:
                                cv.wait()
                            if errors:
                                return
                            targets, cands, probes, ncand, nuniq = built.pop(gi)
                        slots.release()
                        try:
                            t_s0 = _time.perf_counter()
                            for h in (targets, cands, probes):
                                h.rebind(ctx)
                            if cands.n == 0:
                                logger.warning("There are no candidate probes for a "
                                               "grouping of genomes")
                            ids, nrows = engine.setcover_filter(
                                ctx, probes, targets, num_sets=cands.n, universe_p=universe_p_of(gi),
                                **self._model_args())
                            t_s1 = _time.perf_counter()
                            finish(ctx, gi, targets, cands, probes, ncand, nuniq, ids, nrows, res_lock)
                            events.append(("solve lane %d" % li, gi, t_s0 - t_call, t_s1 - t_call))
                            events.append(("finish lane %d" % li, gi, t_s1 - t_call, _time.perf_counter() - t_call))
                        except BaseException as exc:
                            with cv:
                                errors.append(exc)
                                cv.notify_all()
                            slots.release()          # (the producer may be waiting for a slot)
                            try:
                                ctx.sync()           # kernels of this lane may still read the objects closed below
                            except Exception:        # noqa: BLE001 -- the first error is the one to report
                                pass
                        finally:
                            for h in (probes, cands, targets):
                                h.close()
                        if errors:
                            return

                prod = threading.Thread(target=producer, name="catchhip-prefetch")
                threads = [threading.Thread(target=lane, args=(li,), name="catchhip-lane") for li in range(1, nl)]
                prod.start()
                for t in threads:
                    t.start()
                lane(0)
                for t in threads:
                    t.join()
                slots.release()                      # (after an error the builder may be waiting for a slot: into the error flag)
                prod.join()
                for res in built.values():           # built, never consumed (after an error)
                    discard(res)
                if errors:
                    raise errors[0]
            else:
                for chunk in chunks:
                    ctxs = _contexts(len(chunk))
                    specs, held, built = [], [], []
                    try:
                        for ctx, gi in zip(ctxs, chunk):
                            if feed is not None:
                                got, res = next(feed)
                                assert got == gi
                                held.extend(res[:3])
                                targets, cands, probes, ncand, nuniq = res
                                for h in (targets, cands, probes):
                                    h.rebind(ctx)
                            else:
                                targets, cands, probes, ncand, nuniq = build(gi, ctx)
                                held.extend((targets, cands, probes))
                            built.append((targets, cands, probes, ncand, nuniq))
                            if cands.n == 0:
                                logger.warning("There are no candidate probes for a "
                                               "grouping of genomes")
                            specs.append((ctx, probes, targets, cands.n, None, universe_p_of(gi)))
                        results = engine.setcover_filter_many(specs, **self._model_args())
                        for ctx, gi, b, (ids, nrows) in zip(ctxs, chunk, built, results):
                            finish(ctx, gi, b[0], b[1], b[2], b[3], b[4], ids, nrows)
                    finally:
                        for h in reversed(held):
                            h.close()
        finally:
            if pre is not None:
                pre.close()
        timings["pipe_events"] = events
        self.last_timings = timings
        return out

    def _filter_genomes_device_union(self, target_genomes_grouped, probe_length,
                                     probe_stride, seq_length_to_skip=None,
                                     near_duplicate_filter=None,
                                     max_bases=300_000_000, pre_filters=()):
        """_filter_genomes_device for many small groups (the clusters of a
        clustered design): the groups of a chunk share one targets / candidates
        / probes triple that carries group numbers -- duplicates are removed
        inside a group only, the MinHash filter (if any) runs over all groups in
        one pass with each group's own hash functions, the scan pairs a probe
        with its own group's genomes only, and one greedy solve over the
        disjoint union makes every group's own picks in its own order.
        max_bases: bases per instance (a probes object holds < 2^31 bytes of
        probe text: ~21 M candidates of 100 bases, one per 50 target bases; and
        the seed work list of a first scan is sized for 6 seeds per base, 68 B
        each until the rows are built: 300 Mbases -> ~120 GB at most)."""
        assert not self.identify and not self.avoided_genomes
        ngroups = len(target_genomes_grouped)
        out = [[] for _ in range(ngroups)]
        timings = _new_timings(candidates=0, unique_candidates=0)
        ctx = engine.default_context()
        # the clusters of a clustered design may come as views of the genomes' storage (probe_designer.
        # ClusteredFragments: every member a single-sequence genome): sizes, targets and the selected probes' text
        # are then taken from the table, and no Genome / str is made per fragment
        views = target_genomes_grouped if hasattr(target_genomes_grouped, "table") else None
        group_bases = (views.group_bases().tolist() if views is not None
                       else [sum(g.size() for g in grp) for grp in target_genomes_grouped])
        chunks = _pack_under_cap(group_bases, max_bases)

        # Two stages, one chunk apart (CATCHHIP_PREFETCH_DEPTH, 0 = one after the other): a helper thread packs the
        # NEXT chunk's targets, enumerates and de-duplicates its candidates and runs the near-duplicate filter on the
        # upload context (the MinHash filter is ~45 dependent rounds per call: the GPU is mostly waiting), while this
        # thread draws the current chunk's anchors (NumPy, seconds at this scale), scans and solves on the compute
        # context.  The filter's hash functions / sampled positions come from `random`, the anchors from `np.random`:
        # each generator is only ever used by one of the two threads, in chunk order -- the same draws as one after
        # the other.
        depth = int(os.environ.get("CATCHHIP_PREFETCH_DEPTH", "2"))

        import time as _time
        stage_s = dict(pack_s=0.0, candidates_s=0.0, near_duplicates_s=0.0, anchors_s=0.0, solve_s=0.0,
                       ndf_ms=0.0, ndf_probes=0, ndf_pairs=0, ndf_kept=0)
        events = []      # (stage, chunk number, start, end) in seconds since the call began: the pipeline's timeline
        t_call = _time.perf_counter()

        # The front end runs on `workers` threads, each with its own stream (two; test hook CATCHHIP_FRONT_END_WORKERS; the
        # MinHash filter is ~45 dependent rounds of mostly small launches per chunk, 5.3 of the 6.8 s of
        # S5 x 1.0's filters: two of them side by side overlap).  The filter's draws from `random` are made for
        # every chunk first, in chunk order -- the stream of draws one chunk after the other would make.
        workers = max(1, int(_lib.test_env("CATCHHIP_FRONT_END_WORKERS", "2")))
        piped = depth > 0 and len(chunks) > 1
        drawn_ndf = {}
        if near_duplicate_filter is not None and not hasattr(near_duplicate_filter, "_draw_for_groups"):
            # (a filter that cannot draw ahead would draw from the global `random` on two threads at
            # once -- a nondeterministic selection; one builder keeps its draws in chunk order)
            workers = 1
        import threading as _threading
        stage_lock = _threading.Lock()       # (the builders add their stage times and counters side by side)
        if piped and near_duplicate_filter is not None and hasattr(near_duplicate_filter, "_draw_for_groups"):
            for ci, chunk in enumerate(chunks):
                drawn_ndf[ci] = near_duplicate_filter._draw_for_groups(len(chunk))
        chunk_no = {id(c): ci for ci, c in enumerate(chunks)}

        def build(chunk, worker=None):
            bctx = ctx if worker is None else engine.upload_context(index=worker)
            t0 = _time.perf_counter()
            if views is not None:
                genomes = views.table.take(np.concatenate([views.clusters[gi] for gi in chunk]))
                ngen = [len(views.clusters[gi]) for gi in chunk]
            else:
                genomes = [g.seqs for gi in chunk for g in target_genomes_grouped[gi]]
                ngen = [len(target_genomes_grouped[gi]) for gi in chunk]
            targets = engine.Targets(bctx, genomes)
            cands = None
            try:
                targets.set_groups(np.repeat(np.arange(len(chunk)), ngen))
                t1 = _time.perf_counter()
                cands = engine.Candidates(bctx, targets, probe_length, probe_stride, seq_length_to_skip)
                ncand, nuniq = cands.ncandidates, cands.n
                for f in pre_filters:     # (as in _filter_genomes_device; grouped candidates alike)
                    f._apply_to_candidates(cands)
                t2 = _time.perf_counter()
                if near_duplicate_filter is not None:
                    if chunk_no[id(chunk)] in drawn_ndf:
                        near_duplicate_filter._apply_to_grouped_candidates(cands, len(chunk), drawn_ndf[chunk_no[id(chunk)]])
                    else:
                        near_duplicate_filter._apply_to_grouped_candidates(cands, len(chunk))
                    # device time of the filter (HIP events around its launches on this worker's stream) and its work
                    ndf_ms_, cnt = bctx.kernel_ms(engine.PHASE_NDF)[0], bctx.ndf_counters()
                    with stage_lock:
                        stage_s["ndf_ms"] += ndf_ms_
                        stage_s["ndf_probes"] += cnt["probes"]
                        stage_s["ndf_pairs"] += cnt["pairs_compared"]
                        stage_s["ndf_tables"] = cnt["tables"]
                        stage_s["ndf_kept"] += cands.n
                bctx.sync()
                if bctx is not ctx:
                    # handed over here, while this stream is idle: a rebind later would wait for the NEXT chunk's
                    # filter rounds, which this thread queues on the same stream (1.1 s of S5 x 1.0)
                    for h in (targets, cands):
                        h.rebind(ctx)
                t3 = _time.perf_counter()
                with stage_lock:
                    stage_s["pack_s"] += t1 - t0
                    stage_s["candidates_s"] += t2 - t1
                    stage_s["near_duplicates_s"] += t3 - t2
                    events.append(("front", chunk_no[id(chunk)], t0 - t_call, t3 - t_call))
            except BaseException:
                for h in (cands, targets):
                    if h is not None:
                        h.close()
                raise
            return targets, cands, ncand, nuniq

        def discard(res):
            for h in (res[1], res[0]):
                h.close()

        def anchors(n):
            t0 = _time.perf_counter()
            got = _anchors_for_candidates(n, probe_length, self.mismatches, self.lcf_thres, self.kmer_probe_map_k)
            stage_s["anchors_s"] += _time.perf_counter() - t0
            events.append(("anchors", len(events), t0 - t_call, _time.perf_counter() - t_call))
            return got

        # Three stages since round 4 (depth >= 2): front end of chunk i + 2 | anchors of chunk i + 1 | scan and solve
        # of chunk i.  The anchors are NumPy draws and array work (2 s of S5 x 1.0), which release the interpreter
        # lock; np.random is still used by one thread only, in chunk order.
        pre = engine.PrefetchPool(chunks, build, workers, 1, discard) if piped else None
        pre2 = None
        if pre is not None and depth >= 2:
            first = iter(pre)

            def draw(_chunk):
                _c, res = next(first)
                try:
                    return res + (anchors(res[1].n),)
                except BaseException:
                    discard(res)
                    raise
            pre2 = engine.Prefetch(chunks, draw, 1, discard)
        if pre2 is not None:
            feed = iter(pre2)
        elif pre is not None:
            feed = ((c, res + (None,)) for c, res in pre)
        else:
            feed = ((c, build(c) + (None,)) for c in chunks)
        try:
            for chunk, (targets, cands, ncand, nuniq, drawn) in feed:
                logger.info("Groups %d..%d of %d as one instance", chunk[0] + 1, chunk[-1] + 1, ngroups)
                probes = None
                nrows, ids = 0, np.zeros(0, dtype=np.int64)
                try:
                    if views is not None:
                        vt = views.table.take(np.concatenate([views.clusters[gi] for gi in chunk]))
                        if self.coverage <= 1.0:
                            universe_p = [self.coverage] * len(vt)
                        else:      # (:761-792: a number of bases per genome)
                            universe_p = [float(min(self.coverage, n)) / n for n in vt.length.tolist()]
                    else:
                        seqs = [s for gi in chunk for g in target_genomes_grouped[gi] for s in g.seqs]
                        universe_p = [p for gi in chunk
                                      for p in self._make_universe_p(target_genomes_grouped[gi])]
                    timings["candidates"] += ncand
                    timings["unique_candidates"] += nuniq
                    anch = drawn if drawn is not None else anchors(cands.n)
                    t0 = _time.perf_counter()
                    probes = _probes_of_candidates(cands, anch)
                    ids, nrows = engine.setcover_filter(
                        ctx, probes, targets, num_sets=cands.n, universe_p=universe_p, as_array=True,
                        **self._model_args())
                    stage_s["solve_s"] += _time.perf_counter() - t0
                    events.append(("solve", chunk_no[id(chunk)], t0 - t_call, _time.perf_counter() - t_call))
                    # candidate-probe x target-bp of the chunk: every cluster's own candidates x its bases
                    per_group = np.bincount(cands.groups(), minlength=len(chunk)) if cands.n else np.zeros(len(chunk), np.int64)
                    gbases = np.array([group_bases[gi] for gi in chunk], dtype=np.float64)
                    timings["probe_bp_units"] = timings.get("probe_bp_units", 0.0) + float(np.dot(per_group[:len(chunk)], gbases))
                    if ids.size:
                        grp = cands.groups()[ids]
                        pos = cands.positions(ids)
                        which = np.searchsorted(targets.seq_off, pos, side="right") - 1
                        local = pos - targets.seq_off[which]
                        if views is not None:
                            for g, q, o in zip(grp.tolist(), which.tolist(), local.tolist()):
                                out[chunk[g]].append(vt.string(q, o, o + probe_length))
                        else:
                            for g, q, o in zip(grp.tolist(), which.tolist(), local.tolist()):
                                out[chunk[g]].append(seqs[q][o:o + probe_length])
                finally:
                    if pre is not None:
                        ctx.sync()          # (objects built on the upload context go back to its cache: nothing may still read them)
                    for h in (probes, cands, targets):
                        if h is not None:
                            h.close()
                _accumulate(timings, ctx, nrows, int(ids.size))
                events.append(("out", chunk_no[id(chunk)], events[-1][3] if events else 0.0, _time.perf_counter() - t_call))
        finally:
            for p in (pre2, pre):
                if p is not None:
                    p.close()
        timings.update(stage_s)
        timings["union_chunks"] = len(chunks)
        timings["pipe_events"] = events
        self.last_timings = timings
        return out

    def _filter_strs_union(self, input_strs, target_genomes_grouped, todo,
                           selected, timings, max_bases=1 << 30,
                           max_candidates=(1 << 24) - 2):
        """Many independent groups (the clusters of a clustered design) as ONE
        instance per chunk: the groups' candidates and genomes share a probes /
        targets pair with group numbers (catchhip_*_set_groups), so the scan
        only pairs a probe with its own group's genomes; the union of disjoint
        set cover instances solved greedily makes, within every group, that
        group's own picks in its own order (gains never cross groups, ties go to
        the lowest id), and the solver's rounds cover all groups at once.
        Requires equal-length candidates everywhere (then every group would
        choose the same anchor rule and k as the union does, and the union's
        np.random draws are the groups' draws back to back) and no ranks."""
        ctx = engine.default_context()
        packed = _pack_under_cap([sum(g.size() for g in target_genomes_grouped[gi]) for gi in todo], max_bases,
                                 [len(input_strs[gi]) for gi in todo], max_candidates)
        for chunk in ([todo[j] for j in part] for part in packed):
            logger.info("Set cover over groups %d..%d of %d as one instance",
                        chunk[0] + 1, chunk[-1] + 1, len(input_strs))
            counts = np.array([len(input_strs[gi]) for gi in chunk], dtype=np.int64)
            offsets = np.concatenate(([0], np.cumsum(counts)))
            strs = [s for gi in chunk for s in input_strs[gi]]
            ngen = [len(target_genomes_grouped[gi]) for gi in chunk]
            universe_p = [p for gi in chunk
                          for p in self._make_universe_p(target_genomes_grouped[gi])]
            held = []
            try:
                targets, probes = self._open_group(
                    ctx, held, strs, [g for gi in chunk for g in target_genomes_grouped[gi]], assume_unique=True)
                probes.set_groups(np.repeat(np.arange(len(chunk)), counts))
                targets.set_groups(np.repeat(np.arange(len(chunk)), ngen))
                ids, nrows = engine.setcover_filter(ctx, probes, targets, num_sets=len(strs),
                                                    universe_p=universe_p, **self._model_args())
            finally:
                for h in reversed(held):
                    h.close()
            ids = np.asarray(ids, dtype=np.int64)
            grp = np.searchsorted(offsets, ids, side="right") - 1
            for j, gi in enumerate(chunk):
                selected[gi] = (ids[grp == j] - offsets[j]).tolist()
            _accumulate(timings, ctx, nrows, len(ids))


def extension_fraction(n2, covered, p):
    """The coverage fraction to ask of a universe of the REDUCED instance
    (SetCoverFilter._filter_strs_keeping_rows): n2 elements are left of a universe of
    n2 + covered after the fixed probes took theirs, and of the whole universe
    the fraction p was to be covered.  catch/utils/set_cover.py:366-367 lets
    can = int(|U| - p |U|) elements (IEEE double) stay uncovered; the solver
    derives that number from a fraction of ITS universe, so the fraction
    returned makes int(n2 - p' n2) == min(can, n2): exactly 1.0 when nothing may
    stay uncovered, 0.0 when everything left may, else the middle of the
    interval of fractions that give `can` (its ends are half an element away:
    no rounding of a double below 2^32 reaches them)."""
    n = n2 + covered
    can = int(n - p * n)
    if can == 0:
        return 1.0
    if can >= n2:
        return 0.0
    return (n2 - can - 0.5) / n2


def _bases_fraction(n, bases):
    """The fraction to ask of a universe of n elements so that min(bases, n) of
    them are covered: the solver lets int(n - p n) stay uncovered (see
    extension_fraction for the half element)."""
    can = n - min(int(bases), n)
    return 1.0 if can == 0 else (n - can - 0.5) / n


def allocate_budget(gains_per_group, N, keys_per_group=None):
    """How many picks every group keeps when N picks may be kept in all:
    gains_per_group[g][i] = the bases the i-th pick of group g covered first
    (Rows.pick_gains).  A k-way merge: the group whose next pick has the largest
    gain gives that pick, among equal gains the earlier group, until N picks
    are taken or every group is exhausted.  Every group keeps a PREFIX of its
    pick order, whatever the gains look like (partial coverage, ranks and a
    pruned list give sequences that are not monotone).  Only where every
    group's gains are the greedy's own (coverage 1.0, no ranks: they never
    increase) is the merged order the greedy for maximum coverage over all
    groups together, up to ties between groups.  Trailing picks with gain 0 are
    kept only if the budget reaches them.  keys_per_group[g][i] (optional) names
    the i-th pick of group g: a pick whose name the merge has taken already
    (the same probe picked for two datasets, written once) is kept without
    counting towards N, so that N counts distinct names.  Returns the kept
    count per group."""
    import heapq
    if isinstance(N, bool) or not isinstance(N, (int, np.integer)) or N < 1:
        raise ValueError("the probe budget must be an integer >= 1, not %r" % (N,))
    gains = [[int(x) for x in g] for g in gains_per_group]
    kept = [0] * len(gains)
    heap = [(-g[0], gi) for gi, g in enumerate(gains) if g]
    heapq.heapify(heap)
    taken, seen = 0, set()
    while heap and taken < N:
        _neg, gi = heapq.heappop(heap)
        key = (gi, kept[gi]) if keys_per_group is None else keys_per_group[gi][kept[gi]]
        taken += key not in seen
        seen.add(key)
        kept[gi] += 1
        if kept[gi] < len(gains[gi]):
            heapq.heappush(heap, (-gains[gi][kept[gi]], gi))
    return kept


def curve_checkpoints(n, points, extra=()):
    """The pick counts at which a group of n picks is measured: ceil(j n /
    points) for j = 1..points, made distinct, n always among them, and those of
    `extra` that lie in 1..n."""
    ks = {-(-j * n // points) for j in range(1, points + 1)} | {n} | {int(k) for k in extra}
    return sorted(k for k in ks if 1 <= k <= n)


class _Budget:
    """The pick_gains / max_probes part of a _filter_strs_keeping_rows run over all its
    groups: one Rows.pick_gains call per group on the table that went to the
    solver, and with max_probes the cut over all groups once the last one is
    solved -- until then every group's table stays on the device (a second
    small call measures the coverage at the group's cut)."""

    def __init__(self, flt, ctx, ngroups, timings):
        self.flt, self.ctx, self.timings = flt, ctx, timings
        self.kept_tables = {}       # group -> (table, num_sets, ids, denom, covered0)
        flt.last_pick_gains = [np.zeros(0, dtype=np.uint32) for _ in range(ngroups)]
        flt.last_coverage_curve = [[] for _ in range(ngroups)]
        flt.last_budget_kept = [0] * ngroups
        if flt.pick_gains:
            timings.update(gains_ms=0.0, gains_launches=0)

    def holds(self, h):
        return any(h is t[0] for t in self.kept_tables.values())

    def _call(self, table, num_sets, ids, checkpoints, denom, covered0):
        gains, tot, wu, wc = table.pick_gains(num_sets, ids, checkpoints, denom, covered0)
        self.timings["gains_ms"] += table.last_gains_ms              # (summed over the calls of a split list)
        self.timings["gains_launches"] += table.last_gains_launches
        coverable = int(np.sum(denom))
        rows = [(int(k), int(t), coverable, int(u), int(c), int(denom[u]) if u >= 0 else 0)
                for k, t, u, c in zip(checkpoints, tot, wu, wc)]
        return gains, rows

    def group(self, gi, table, num_sets, ids, denom, covered0):
        flt = self.flt
        flt.last_budget_kept[gi] = len(ids)
        if len(ids) == 0:
            return
        denom = np.asarray(denom, dtype=np.int64)
        covered0 = None if covered0 is None else np.asarray(covered0, dtype=np.int64)
        flt.last_pick_gains[gi], flt.last_coverage_curve[gi] = self._call(
            table, num_sets, ids, curve_checkpoints(len(ids), flt.curve_points), denom, covered0)
        if flt.max_probes is not None:
            self.kept_tables[gi] = (table, num_sets, list(ids), denom, covered0)

    def release(self):
        """Closes the tables held for the cut; the filter calls it whether its
        groups went through or one of them raised."""
        for t in self.kept_tables.values():
            t[0].close()
        self.kept_tables = {}

    def finish(self, selected, input_strs):
        """The cut (max_probes): selected[group] becomes the prefix kept.  The
        budget counts distinct probe sequences: the designer writes a probe
        picked for two groups once, so sum(last_budget_kept), which counts
        picks, can exceed max_probes."""
        flt = self.flt
        try:
            if flt.max_probes is None:
                return
            kept = allocate_budget(flt.last_pick_gains, flt.max_probes,
                                   [[strs[i] for i in ids] for strs, ids in zip(input_strs, selected)])
            for gi, k in enumerate(kept):
                curve = flt.last_coverage_curve[gi]
                if gi in self.kept_tables and k >= 1 and all(row[0] != k for row in curve):
                    table, num_sets, ids, denom, covered0 = self.kept_tables[gi]
                    _g, rows = self._call(table, num_sets, ids, [k], denom, covered0)
                    flt.last_coverage_curve[gi] = sorted(curve + rows)
                self.timings["picks"] -= len(selected[gi]) - k
                selected[gi] = selected[gi][:k]
            flt.last_budget_kept = kept
        finally:
            self.release()


def _prune(ctx, rows, num_sets, ids, depth, fixed_rows, timings):
    """Rows.prune of a group's picks (SetCoverFilter(prune_redundant=True)) ->
    (the picks kept, the picks dropped); its device time, launches and rounds
    and the number dropped are added to `timings`."""
    kept, removed = rows.prune(num_sets, ids, depth, fixed_rows)
    ms, nl = ctx.kernel_ms(engine.PHASE_ROWS) if len(ids) else (0.0, 0)
    timings["prune_ms"] = timings.get("prune_ms", 0.0) + ms
    timings["prune_launches"] = timings.get("prune_launches", 0) + nl
    timings["prune_rounds"] = timings.get("prune_rounds", 0) + rows.last_prune_rounds
    timings["pruned"] = timings.get("pruned", 0) + len(removed)
    return kept, removed


def _solver_fractions(universe_p):
    """What the solvers take as universe_p: None selects their full-coverage
    path when every universe is to be covered whole."""
    return None if all(p == 1.0 for p in universe_p) else universe_p


def _warn_less_than_ideal(gi, ranks, ids):
    """The reference's warning (:176-186) when picks of group `gi` have a rank
    above the best one."""
    num_bad = int(np.count_nonzero(ranks[ids] > 0)) if len(ids) else 0
    if num_bad > 0:
        logger.warning(("Group %d: forced to choose %d less-than-ideal "
                        "probe%s (i.e., probes that 'hit' more than "
                        "one grouping during identification or probes "
                        "that cover an avoided genome)"), gi + 1,
                       num_bad, "" if num_bad == 1 else "s")


def _pack_under_cap(sizes, cap, counts=None, count_cap=None):
    """Consecutive items 0 .. len(sizes) - 1 in chunks, each as long as it can
    be with sum(sizes) <= cap (and, given counts, sum(counts) <= count_cap); an
    item that alone exceeds a cap is a chunk of its own.  -> [[item]]."""
    chunks = []
    for i, size in enumerate(sizes):
        count = counts[i] if counts is not None else 0
        if chunks and total + size <= cap and (counts is None or ncount + count <= count_cap):
            chunks[-1].append(i)
            total, ncount = total + size, ncount + count
        else:
            chunks.append([i])
            total, ncount = size, count
    return chunks


def _lpt(costs, nbins):
    from catch_amd import parallel
    return parallel.lpt_assign(costs, nbins)


def _new_timings(**extra):
    """A fresh last_timings: the keys every path of the filter reports, and
    those of `extra`."""
    return dict(scan_ms=0.0, rows_ms=0.0, greedy_ms=0.0, picks=0, rows=0,
                scan_launches=0, greedy_launches=0, **extra)


_SCAN_PHASES = (("scan_ms", engine.PHASE_SCAN), ("verify_ms", engine.PHASE_VERIFY),
                ("rows_ms", engine.PHASE_ROWS))
_GREEDY_PHASES = (("greedy_ms", engine.PHASE_GREEDY), ("rounds_ms", engine.PHASE_GREEDY_ROUNDS),
                  ("claim_ms", engine.PHASE_CLAIM))


def _add_phase_times(timings, ctx, phases):
    """Adds the device time (HIP events) and the launches that the context's
    last call spent in each (name_ms, phase) to timings[name_ms] and
    timings[name_launches]."""
    for name, ph in phases:
        ms, nl = ctx.kernel_ms(ph)
        timings[name] = timings.get(name, 0.0) + ms
        ln = name.replace("_ms", "_launches")
        timings[ln] = timings.get(ln, 0) + nl


def _accumulate(timings, ctx, nrows, npicks):
    """Adds the device times and work counters of the context's last fused
    filter call to `timings`."""
    _add_phase_times(timings, ctx, _SCAN_PHASES + _GREEDY_PHASES)
    timings["rows"] = timings.get("rows", 0) + nrows
    timings["picks"] = timings.get("picks", 0) + npicks
    for k, v in ctx.counters().items():
        if k not in ("picks", "_"):
            timings[k] = timings.get(k, 0) + v


def _chunks_by_size(todo, size_of, width):
    """Groups in flight together.  Large groups (>= CATCHHIP_BIG_GROUP_BASES,
    default 8 Mbases) fill the GPU on their own and run one at a time, largest
    first (their kernels only get in each other's way: four S4 groups in flight
    took 498 ms per pass against 333 ms one after the other); the small ones
    run `width` at a time on their own streams."""
    import os
    big_bases = int(os.environ.get("CATCHHIP_BIG_GROUP_BASES", str(8_000_000)))
    big = [[gi] for gi in todo if size_of(gi) >= big_bases]
    small = [gi for gi in todo if size_of(gi) < big_bases]
    return big + [small[i:i + width] for i in range(0, len(small), width)]


_extra_ctxs = {}


def _devices():
    """Devices the groups in flight are spread over.  Default: the default
    context's device only (one process per GPU, as torchrun launches the
    bench).  CATCHHIP_DEVICES=all or a comma-separated list lets ONE process
    use several GPUs for independent groups (first row: whole
    groups to GPUs, no collective): every context has its own device, stream
    and allocator partition, and catchhip_setcover_filter_many already runs
    one host thread per context."""
    import os
    first = engine.default_context().device
    spec = os.environ.get("CATCHHIP_DEVICES", "")
    if not spec:
        return [first]
    if spec == "all":
        devs = list(range(engine.device_count()))
    else:
        devs = [int(x) for x in spec.split(",") if x.strip() != ""]
    devs = [d for d in devs if 0 <= d < engine.device_count()]
    if first in devs:                      # the default context keeps slot 0
        devs.remove(first)
    return [first] + devs


def _contexts(n):
    """The default context plus cached extra ones, one per group in flight,
    round-robin over _devices()."""
    first = engine.default_context()
    devs = _devices()
    out = [first]
    for i in range(1, n):
        dev = devs[i % len(devs)]
        key = (dev, i // len(devs))
        if key not in _extra_ctxs:
            _extra_ctxs[key] = engine.Context(dev)
        out.append(_extra_ctxs[key])
    return out


def _anchors_for_candidates(n, probe_length, mismatches, lcf_thres, map_k):
    """(k, "table" | "draws" | "entries", payload) for the device front end's n
    equal-length candidates: the pigeonhole table (payload None), random anchors
    as their np.random draws (the device sorts and de-duplicates them), or -- for
    probes longer than 256 + k -- as host-made entries.  The same np.random draws
    in all three forms."""
    if probe_length - map_k + 1 <= 256:
        k, draws = probe.anchor_draws_equal_length(n, probe_length, mismatches, lcf_thres,
                                                   min_k=map_k, k=map_k)
        return (k, "table", None) if draws is None else (k, "draws", draws)
    k, ep, eo = probe.anchor_entries_equal_length(n, probe_length, mismatches, lcf_thres,
                                                  min_k=map_k, k=map_k)
    return (k, "table", None) if ep is None else (k, "entries", (ep, eo))


def _probes_of_candidates(cands, anchors):
    k, kind, payload = anchors
    if kind == "draws":
        return cands.probes_from_draws(k, payload)
    if kind == "entries":
        return cands.probes(k, payload[0], payload[1])
    return cands.probes(k)
