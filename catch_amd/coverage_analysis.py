"""Coverage analysis of a probe set on the MI355X: drop-in for
catch/coverage_analysis.py (Analyzer, :66-600).

The one expensive step -- finding every range of every target genome (and of
its reverse complement) that some probe covers,
`probe.find_probe_covers_in_sequence(sequence, merge_overlapping=False)` per
sequence (:183-280) -- is one catchhip_cover_ranges call per strand over all
genomes at once (every sequence its own universe); the statistics the
reference derives from those ranges (:282-335) are reduced on the device too (catchhip_rows_stats: bases
covered, summed range lengths, sequences per probe), so a report over thousands
of genomes never brings the row table to the host.  The sliding-window depth
(:337-411) is computed on the device as well (catchhip_rows_window_depth, one
scan per strand on first use of `sliding_coverage` or its writer): what comes
back is one integer sum and one base count per window, never a range.
`target_covers` is fetched on first use.  Where the probes do not reach is read
out on the device too (`uncovered_regions` and its writers,
catchhip_rows_uncovered: one scan per strand, only the regions come back).
Same constructor, attributes (`target_covers`, `bp_covered`,
`average_coverage`, `sliding_coverage`, `probe_map_counts`) and writers.

Not supported (raises NotImplementedError): `custom_cover_range_fn`.
"""
from collections import Counter
import logging

import numpy as np

from catch_amd import _lib
from catch_amd import engine
from catch_amd import probe

logger = logging.getLogger(__name__)

_RC = str.maketrans("ACGT", "TGCA")


class Analyzer:
    def __init__(self, probes, mismatches, lcf_thres, target_genomes,
                 target_genomes_names=None, island_of_exact_match=0,
                 custom_cover_range_fn=None, cover_extension=0,
                 kmer_probe_map_k=10, rc_too=True, either_strand=False,
                 target_regions=None):
        if custom_cover_range_fn is not None:
            raise NotImplementedError(
                "custom hybridization functions cannot run on the GPU path")
        # either_strand (not an argument of the reference's class): the probes capture a locus whichever strand of it
        # was deposited (design --either-strand).  The analysed list is then the probes followed by their reverse
        # complements, against the forward strand only: bases covered, average depth, sliding-window depth and
        # uncovered regions describe the forward strand's loci under either orientation of a probe.  probe_map_counts
        # folds each reverse complement's count onto its probe: a sequence that both orientations map to counts twice.
        if either_strand and rc_too:
            raise ValueError("either_strand analyses the forward strand under both orientations of the probes; "
                             "rc_too must be False with it")
        self.either_strand = bool(either_strand)
        # the bases that were to be covered at all (catch_amd.target_regions.TargetRegions, or None: every base; not
        # an argument of the reference's class): uncovered_regions() then lists runs of wanted bases only.  Everything
        # else the analyzer reports keeps describing whole genomes.
        self.target_regions = target_regions
        self.probes = probes
        self._analysed = (list(probes) + [p.reverse_complement() for p in probes]) if self.either_strand else probes
        self.target_genomes = target_genomes
        if target_genomes_names:
            if len(target_genomes_names) != len(target_genomes):
                raise ValueError(("Number of target genome names must be same "
                                  "as the number of target genomes"))
            self.target_genomes_names = target_genomes_names
        else:
            self.target_genomes_names = ["Group %d" % i
                                         for i in range(len(target_genomes))]
        self.mismatches = mismatches
        self.lcf_thres = lcf_thres
        self.island_of_exact_match = island_of_exact_match
        self.cover_extension = cover_extension
        self.kmer_probe_map_k = kmer_probe_map_k
        self.rc_too = rc_too
        self._covers = None
        self._sliding = None
        self._windows = None
        self._window = (50, 25)
        self._scan_inputs = None
        self._np_state = None
        self._uncovered = {}
        self.uncovered_summary = {}
        self.last_uncovered_ms = 0.0      # device time of the last uncovered_regions() that went to the device, both strands

    def _iter_target_genomes(self, groups=None):
        """groups: only these groupings, in the order given (the rows of one
        dataset of a report that several analyzers share; None = all)."""
        for i in (range(len(self.target_genomes)) if groups is None else groups):
            for j, gnm in enumerate(self.target_genomes[i]):
                yield i, j, gnm, False
                if self.rc_too:
                    yield i, j, gnm, True

    # ------------------------------------------------------------------
    def _strand_targets(self, ctx, flat, rc):
        """All sequences of all genomes as one targets object, every sequence
        its own universe (ranges stay per sequence); plus, per sequence, the
        genome it belongs to and its offset inside the genome."""
        seqs, owner_of_seq, offset_of_seq = [], [], []
        for g, (_i, _j, gnm) in enumerate(flat):
            so_far = 0
            for s in gnm.seqs:
                seqs.append([s[::-1].translate(_RC) if rc else s])
                owner_of_seq.append(g)
                offset_of_seq.append(so_far)
                so_far += len(s)
        return (engine.Targets(ctx, seqs), np.asarray(owner_of_seq, dtype=np.int64),
                np.asarray(offset_of_seq, dtype=np.int64))

    def _scan(self, ctx, probes_dev, targets):
        return engine.Rows.scan(ctx, probes_dev, targets, self.mismatches,
                                self.lcf_thres, self.island_of_exact_match,
                                self.cover_extension, engine.SCAN_AUTO, merge=False)

    def _flat_genomes(self):
        return [(i, j, gnm) for i, grp in enumerate(self.target_genomes)
                for j, gnm in enumerate(grp)]

    def _find_covers_in_target_genomes(self):
        """One scan per strand over all genomes (every distinct range of every
        probe, nothing merged: find_probe_covers_in_sequence(...,
        merge_overlapping=False), :183-280).  The row table stays on the device;
        what the report needs is reduced there (catchhip_rows_stats):
          self.bp_covered[i][j][rc]   bases covered by at least one probe (:282-302)
          self._total_covered[i][j][rc]  sum of the ranges' lengths (:318-320)
          self.probe_map_counts[p]    sequences probe p maps to, forward strand (:255-258)
        self.target_covers is fetched on first use (it needs every range on the
        host); self.sliding_coverage is computed on first use, on the device."""
        logger.info("Finding probe covers across target genomes")
        self.probe_map_counts = Counter()
        self.bp_covered, self._total_covered = {}, {}
        for i, j, _gnm, rc in self._iter_target_genomes():
            for d in (self.bp_covered, self._total_covered):
                d.setdefault(i, {}).setdefault(j, {False: None, True: None})[rc] = 0
        self._covers = None
        self._sliding = self._windows = None
        self._uncovered = {}
        strs = [p.seq_str for p in self._analysed]
        flat = self._flat_genomes()
        self._scan_inputs = None
        if not strs or not flat:
            return
        ctx = engine.default_context()
        # (random anchors draw from np.random: _map_count_order replays the draws)
        self._np_state = np.random.get_state()
        self._scan_inputs = probe.anchor_table(
            strs, self.mismatches, self.lcf_thres,
            min_k=self.kmer_probe_map_k, k=self.kmer_probe_map_k)
        k, uniq, owner, ep, eo = self._scan_inputs
        probes_dev = engine.Probes(ctx, uniq, owner, ep, eo, k)
        try:
            for rc in ((False, True) if self.rc_too else (False,)):
                targets, owner_of_seq, _off = self._strand_targets(ctx, flat, rc)
                try:
                    rows = self._scan(ctx, probes_dev, targets)
                    total_len, union_len, per_probe = rows.stats(
                        targets.ngenomes, len(strs) if not rc else 0)
                    rows.close()
                finally:
                    targets.close()
                tot = np.bincount(owner_of_seq, weights=total_len.astype(np.float64),
                                  minlength=len(flat)).astype(np.int64)
                uni = np.bincount(owner_of_seq, weights=union_len.astype(np.float64),
                                  minlength=len(flat)).astype(np.int64)
                for g, (i, j, _gnm) in enumerate(flat):
                    self.bp_covered[i][j][rc] = int(uni[g])
                    self._total_covered[i][j][rc] = int(tot[g])
                if not rc:
                    self._fold_map_counts(per_probe)
        finally:
            probes_dev.close()

    def _fold_map_counts(self, per_probe):
        """per_probe[a] = the sequences entry `a` of the analysed list maps to,
        added to probe_map_counts; under either_strand entry n + i, the reverse
        complement of probe i, counts for probe i (a sequence that both
        orientations map to counts twice)."""
        n = len(self.probes)
        for a in np.nonzero(per_probe)[0]:
            self.probe_map_counts[self.probes[a % n if self.either_strand else a]] += int(per_probe[a])

    @property
    def target_covers(self):
        """target_covers[i][j][rc] = sorted list of (start, end) in genome
        coordinates (chromosomes offset by the lengths before them), one entry
        per distinct range of every probe.  Fetched from the device on first
        use (a second scan: the report itself does not need them)."""
        if self._covers is None:
            self._covers = self._fetch_covers()
        return self._covers

    def _fetch_covers(self):
        covers = {}
        for i, j, _gnm, rc in self._iter_target_genomes():
            covers.setdefault(i, {}).setdefault(j, {False: None, True: None})[rc] = []
        flat = self._flat_genomes()
        if self._scan_inputs is None:
            return covers
        ctx = engine.default_context()
        k, uniq, owner, ep, eo = self._scan_inputs
        probes_dev = engine.Probes(ctx, uniq, owner, ep, eo, k)
        try:
            for rc in ((False, True) if self.rc_too else (False,)):
                targets, owner_of_seq, offset_of_seq = self._strand_targets(ctx, flat, rc)
                try:
                    rows = self._scan(ctx, probes_dev, targets)
                    _sid, univ, st, en = rows.fetch()
                    rows.close()
                finally:
                    targets.close()
                gidx = owner_of_seq[univ] if univ.size else univ.astype(np.int64)
                a = st + (offset_of_seq[univ] if univ.size else 0)
                b = en + (offset_of_seq[univ] if univ.size else 0)
                order = np.lexsort((b, a, gidx))
                gidx, a, b = gidx[order], a[order], b[order]
                bounds = np.searchsorted(gidx, np.arange(len(flat) + 1))
                for g, (i, j, _gnm) in enumerate(flat):
                    lo, hi = bounds[g], bounds[g + 1]
                    covers[i][j][rc] = list(zip(a[lo:hi].tolist(), b[lo:hi].tolist()))
        finally:
            probes_dev.close()
        return covers

    def _compute_bp_covered_in_target_genomes(self):
        """Done on the device by _find_covers_in_target_genomes."""

    def _compute_average_coverage_in_target_genomes(self):
        self.average_coverage = {}
        for i, j, gnm, rc in self._iter_target_genomes():
            total_covered = self._total_covered[i][j][rc]
            self.average_coverage.setdefault(i, {}).setdefault(
                j, {False: None, True: None})[rc] = (
                float(total_covered) / gnm.size(False),
                float(total_covered) / gnm.size(True))

    def _compute_sliding_coverage_in_target_genomes(self, window_length,
                                                    window_stride):
        """:337-411: average depth in windows; keys are window middles.
        Computed on first use of self.sliding_coverage or of its writer."""
        self._window = (window_length, window_stride)
        self._sliding = self._windows = None

    def _window_tables(self):
        """Per strand (keys, values, win_off): the windows of flat genome g are
        win_off[g]:win_off[g + 1], keys[w] the window's middle as the reference
        reports it (:401-408) and values[w] its average depth.  One scan per
        strand; the depth, its prefix sums and the window sums stay on the
        device (Rows.window_depth), which returns an integer sum and a base
        count per window: float(sum) / count is np.average of the reference's
        uint16 slice (:409-410), whose sum is exact in float64."""
        if self._windows is not None:
            return self._windows
        window_length, window_stride = self._window
        flat = self._flat_genomes()
        sizes = np.asarray([gnm.size(False) for _i, _j, gnm in flat], dtype=np.int64)
        span_first = np.zeros(len(flat) + 1, dtype=np.int64)
        np.cumsum([len(gnm.seqs) for _i, _j, gnm in flat], out=span_first[1:])
        strands = (False, True) if self.rc_too else (False,)
        device = {}
        if self._scan_inputs is not None:
            ctx = engine.default_context()
            k, uniq, owner, ep, eo = self._scan_inputs
            probes_dev = engine.Probes(ctx, uniq, owner, ep, eo, k)
            try:
                for rc in strands:
                    targets, _owner, _off = self._strand_targets(ctx, flat, rc)
                    try:
                        rows = self._scan(ctx, probes_dev, targets)
                        device[rc] = rows.window_depth(span_first, window_length,
                                                       window_stride)
                        rows.close()
                    finally:
                        targets.close()
            finally:
                probes_dev.close()
        # the reported start of every window, for all genomes at once (:401-407)
        per = -(-sizes // window_stride)
        win_off = np.zeros(len(flat) + 1, dtype=np.int64)
        np.cumsum(per, out=win_off[1:])
        n = np.repeat(sizes, per)
        start = (np.arange(win_off[-1], dtype=np.int64) - np.repeat(win_off[:-1], per)) * window_stride
        start = np.where(start + window_length > n, n - window_length, start)
        keys = start + (window_length / 2)
        self._windows = {}
        for rc in strands:
            if rc in device:
                sums, counts, off = device[rc]
                assert np.array_equal(off, win_off)
                values = sums.astype(np.float64) / counts
            else:       # no probes: nothing is covered
                values = np.zeros(keys.size, dtype=np.float64)
            self._windows[rc] = (keys, values, win_off)
        return self._windows

    def _host_sliding_coverage(self):
        """The same on the host from the fetched ranges, base by base and window
        by window: the path the device computation is tested against
        (CATCHHIP_ANALYSIS_HOST_WINDOWS=1, a test hook)."""
        window_length, window_stride = self._window
        sliding = {}
        for i, j, gnm, rc in self._iter_target_genomes():
            covers = self.target_covers[i][j][rc]
            n = gnm.size(False)
            diff = np.zeros(n + 1, dtype=np.int64)
            if covers:
                arr = np.asarray(covers, dtype=np.int64)
                np.add.at(diff, arr[:, 0], 1)
                np.add.at(diff, arr[:, 1], -1)
            # the reference stores the depth as uint16
            counts = np.cumsum(diff[:n]).astype(np.uint16)
            out = {}
            for window_start in np.arange(0, n, window_stride):
                window_end = window_start + window_length
                if window_end > n:
                    window_end = n
                    window_start = window_end - window_length
                middle = window_start + (window_length / 2)
                out[middle] = np.average(counts[window_start:window_end])
            sliding.setdefault(i, {}).setdefault(
                j, {False: None, True: None})[rc] = out
        return sliding

    @staticmethod
    def _host_windows():
        return _lib.test_env("CATCHHIP_ANALYSIS_HOST_WINDOWS", "0") not in ("", "0")

    @property
    def sliding_coverage(self):
        if self._sliding is None:
            if self._host_windows():
                self._sliding = self._host_sliding_coverage()
                return self._sliding
            tables = self._window_tables()
            self._sliding = {}
            for g, (i, j, _gnm) in enumerate(self._flat_genomes()):
                for rc, (keys, values, win_off) in tables.items():
                    lo, hi = win_off[g], win_off[g + 1]
                    self._sliding.setdefault(i, {}).setdefault(
                        j, {False: None, True: None})[rc] = dict(
                            zip(keys[lo:hi].tolist(), values[lo:hi].tolist()))
        return self._sliding

    def run(self, window_length=50, window_stride=25):
        self._find_covers_in_target_genomes()
        self._compute_bp_covered_in_target_genomes()
        self._compute_average_coverage_in_target_genomes()
        self._compute_sliding_coverage_in_target_genomes(window_length,
                                                         window_stride)

    # ------------------------------------------------------------------
    def uncovered_regions(self, min_depth=1, min_length=1, min_unambig=1):
        """{i: {j: {rc: [(seq_index, start, end, unambig), ...]}}}: the maximal
        runs of bases, inside one sequence, that fewer than min_depth cover
        ranges hold, by (sequence, start); start and end are 0-based, half-open,
        within the sequence as scanned (for rc: the reverse-complemented
        sequence, as in the sliding-window file), unambig = the run's bases that
        are A, C, G or T.  Reported are the runs of min_length bases and more
        with at least min_unambig unambiguous ones.  Also fills
        self.uncovered_summary[i][j][rc] = (regions, bases, longest).  After
        run(); one scan per strand, the row table stays on the device
        (Rows.uncovered) and only the regions come back.  With no probes every
        sequence that passes the filters is one region.  With target_regions the
        runs are runs of WANTED bases: an unwanted base ends a run as a covered
        one does (one BaseMask per strand; with no probes every wanted interval
        that passes the filters is one region)."""
        key = (int(min_depth), int(min_length), int(min_unambig))
        if key not in self._uncovered:
            self._uncovered[key] = self._find_uncovered(*key)
        regions, self.uncovered_summary = self._uncovered[key]
        return regions

    def _find_uncovered(self, min_depth, min_length, min_unambig):
        regions, summary = {}, {}
        for i, j, _gnm, rc in self._iter_target_genomes():
            regions.setdefault(i, {}).setdefault(j, {False: None, True: None})[rc] = []
            summary.setdefault(i, {}).setdefault(j, {False: None, True: None})[rc] = (0, 0, 0)
        flat = self._flat_genomes()
        if not flat:
            return regions, summary
        ctx = engine.default_context()
        first_seq = np.zeros(len(flat) + 1, dtype=np.int64)
        np.cumsum([len(gnm.seqs) for _i, _j, gnm in flat], out=first_seq[1:])
        probes_dev = None
        if self._scan_inputs is not None:
            k, uniq, owner, ep, eo = self._scan_inputs
            probes_dev = engine.Probes(ctx, uniq, owner, ep, eo, k)
        self.last_uncovered_ms = 0.0
        try:
            for rc in ((False, True) if self.rc_too else (False,)):
                # (the targets stay until the regions are back: the kernel counts their A, C, G, T)
                targets, owner_of_seq, _off = self._strand_targets(ctx, flat, rc)
                try:
                    if probes_dev is not None:
                        rows = self._scan(ctx, probes_dev, targets)
                    else:       # no probes: a table without rows over the same sequences
                        rows = engine.Rows.from_host(ctx, [], [], [], [], np.diff(targets.seq_off))
                    mask = None
                    try:
                        if self.target_regions is not None:     # one mask per strand, a universe per sequence
                            mask = engine.BaseMask(ctx, np.diff(targets.seq_off),
                                                   *self.target_regions.sequence_intervals(flat, rc))
                        univ, st, en, ua, per = rows.uncovered(targets, min_depth, min_length, min_unambig, mask=mask)
                        self.last_uncovered_ms += rows.last_uncovered_ms
                    finally:
                        if mask is not None:
                            mask.close()
                        rows.close()
                finally:
                    targets.close()
                bounds = np.searchsorted(univ, first_seq)       # (the regions come by (sequence, start))
                seq = univ.astype(np.int64) - (first_seq[owner_of_seq[univ]] if univ.size else 0)
                for g, (i, j, _gnm) in enumerate(flat):
                    lo, hi = bounds[g], bounds[g + 1]
                    regions[i][j][rc] = list(zip(seq[lo:hi].tolist(), st[lo:hi].tolist(), en[lo:hi].tolist(),
                                                 ua[lo:hi].tolist()))
                    p = per[first_seq[g]:first_seq[g + 1]]
                    summary[i][j][rc] = ((int(p[:, 0].sum()), int(p[:, 1].sum()), int(p[:, 2].max()))
                                         if p.size else (0, 0, 0))
        finally:
            if probes_dev is not None:
                probes_dev.close()
        return regions, summary

    _UNCOVERED_HEADER = ["Genome", "Sequence", "Start", "End", "Length", "Unambig bases"]

    @staticmethod
    def _sequence_name(gnm, seq_index):
        """The sequence's name in gnm.chrs when it has one, else its index."""
        return list(gnm.chrs.keys())[seq_index] if gnm.chrs else seq_index

    def write_uncovered_regions(self, fn, min_depth=1, min_length=1, min_unambig=1):
        with open(fn, "w") as f:
            f.write("\t".join(self._UNCOVERED_HEADER) + "\n")
            self._write_uncovered_rows(f, None, min_depth, min_length, min_unambig)

    def _write_uncovered_rows(self, f, groups=None, min_depth=1, min_length=1, min_unambig=1):
        regions = self.uncovered_regions(min_depth, min_length, min_unambig)
        for i, j, gnm, rc in self._iter_target_genomes(groups):
            header = self._row_header(i, j, rc)
            names = list(gnm.chrs.keys()) if gnm.chrs else None
            f.write("".join("%s\t%s\t%d\t%d\t%d\t%d\n" % (header, names[s] if names else s, a, b, b - a, u)
                            for s, a, b, u in regions[i][j][rc]))

    def write_uncovered_fasta(self, fn, min_depth=1, min_length=1, min_unambig=1):
        """The uncovered regions of the forward strand as FASTA records:
        >{row header}|{sequence}|{start}-{end}, then that slice of the sequence."""
        with open(fn, "w") as f:
            self._write_uncovered_fasta_rows(f, None, min_depth, min_length, min_unambig)

    def _write_uncovered_fasta_rows(self, f, groups=None, min_depth=1, min_length=1, min_unambig=1):
        regions = self.uncovered_regions(min_depth, min_length, min_unambig)
        for i, j, gnm, rc in self._iter_target_genomes(groups):
            if rc:
                continue
            header = self._row_header(i, j, rc)
            for s, a, b, _u in regions[i][j][rc]:
                f.write(">%s|%s|%d-%d\n%s\n" % (header, self._sequence_name(gnm, s), a, b, gnm.seqs[s][a:b]))

    def log_uncovered_summary(self, label="", min_depth=1, min_length=1, min_unambig=1):
        """One line per dataset under --verbose: regions, uncovered bases, longest (over every genome and strand)."""
        self.uncovered_regions(min_depth, min_length, min_unambig)
        for i in range(len(self.target_genomes)):
            triples = [t for j in self.uncovered_summary.get(i, {}).values() for t in j.values() if t is not None]
            logger.info("%s%s: %d uncovered regions, %d uncovered bases, longest %d", label,
                        self.target_genomes_names[i], sum(t[0] for t in triples), sum(t[1] for t in triples),
                        max([t[2] for t in triples] + [0]))

    # ------------------------------------------------------------------
    def _row_header(self, i, j, rc):
        h = "%s, genome %d" % (self.target_genomes_names[i], j)
        return h + " (rc)" if rc else h

    _TSV_HEADER = ["Genome", "Num bases covered", "Frac bases covered",
                   "Frac bases covered over unambig", "Average coverage/depth",
                   "Average coverage/depth over unambig"]

    def _data_matrix_rows(self, groups=None):
        data = []
        for i, j, gnm, rc in self._iter_target_genomes(groups):
            bp_covered = self.bp_covered[i][j][rc]
            avg_all, avg_unambig = self.average_coverage[i][j][rc]
            data.append([self._row_header(i, j, rc), bp_covered,
                         float(bp_covered) / gnm.size(False),
                         float(bp_covered) / gnm.size(True),
                         avg_all, avg_unambig])
        return data

    def write_data_matrix_as_tsv(self, fn):
        with open(fn, "w") as f:
            for row in [self._TSV_HEADER] + self._data_matrix_rows():
                f.write("\t".join(str(entry) for entry in row) + "\n")

    _TABLE_HEADER = ["Genome", "Num bases covered\n[over unambig]",
                     "Average coverage/depth\n[over unambig]"]

    def _make_data_matrix_string(self, groups=None):
        data = [self._TABLE_HEADER] if groups is None else []
        for i, j, gnm, rc in self._iter_target_genomes(groups):
            bp_covered = self.bp_covered[i][j][rc]
            frac_all = float(bp_covered) / gnm.size(False)
            frac_unambig = float(bp_covered) / gnm.size(True)
            all_str = "<0.01%" if frac_all < 0.0001 else "{0:.2%}".format(frac_all)
            unambig_str = ("<0.01%" if frac_unambig < 0.0001
                           else "{0:.2%}".format(frac_unambig))
            bp_str = "%d (%s) [%s]" % (bp_covered, all_str, unambig_str)
            avg_all, avg_unambig = self.average_coverage[i][j][rc]
            a = "<0.01" if avg_all < 0.01 else "{0:.2f}".format(avg_all)
            u = "<0.01" if avg_unambig < 0.01 else "{0:.2f}".format(avg_unambig)
            data.append([self._row_header(i, j, rc), bp_str, "%s [%s]" % (a, u)])
        return data

    def print_analysis(self):
        print("NUMBER OF PROBES: %d" % len(self.probes))
        print()
        print_table(self._make_data_matrix_string())

    def write_sliding_window_coverage(self, fn):
        with open(fn, "w") as f:
            self._write_sliding_rows(f)

    def _write_sliding_rows(self, f, groups=None):
        if self._host_windows():
            for i, j, _gnm, rc in self._iter_target_genomes(groups):
                header = self._row_header(i, j, rc)
                cov = self.sliding_coverage[i][j][rc]
                for pos in sorted(cov.keys()):
                    f.write("\t".join(str(x) for x in [header, pos, cov[pos]]) + "\n")
            return
        # Straight from the window tables, genome by genome.  A genome's keys
        # ascend; the windows that stretch past its end share one key and one
        # value (one dict entry in the reference): the last of a run is written.
        tables = self._window_tables()
        flat_index = {(i, j): g for g, (i, j, _gnm) in enumerate(self._flat_genomes())}
        for i, j, _gnm, rc in self._iter_target_genomes(groups):
            header = self._row_header(i, j, rc)
            keys, values, win_off = tables[rc]
            g = flat_index[(i, j)]
            k, v = keys[win_off[g]:win_off[g + 1]], values[win_off[g]:win_off[g + 1]]
            if not k.size:
                continue
            last = np.append(k[1:] != k[:-1], True)
            f.write("".join("%s\t%s\t%s\n" % (header, pos, val) for pos, val in
                            zip(k[last].tolist(), v[last].tolist())))

    def _map_count_order(self):
        """The probes that map somewhere (as indices into self.probes), in the
        order the reference first meets them (:222-250: genomes and sequences
        in order, inside a sequence by the position of the first accepted k-mer,
        at one position in the order the k-mer map lists its entries) -- the
        order of its probe_map_counts, which a Counter keeps.  One more scan of
        the forward strand (catchhip_cover_scan_first_seen); per probe the
        first sequence and the key inside it are picked on the device."""
        if self._scan_inputs is None:
            return []
        strs = [p.seq_str for p in self._analysed]
        state = np.random.get_state()
        np.random.set_state(self._np_state)
        try:
            k, uniq, owner, ep, eo, draws = probe.anchor_table(
                strs, self.mismatches, self.lcf_thres, min_k=self.kmer_probe_map_k,
                k=self.kmer_probe_map_k, with_draws=True)
        finally:
            np.random.set_state(state)
        order = probe.anchor_order(self._analysed, strs, uniq, ep, eo, draws, k)
        ctx = engine.default_context()
        probes_dev = engine.Probes(ctx, uniq, owner, ep, eo, k)
        try:
            targets, _owner, _off = self._strand_targets(ctx, self._flat_genomes(), False)
            try:
                rows = engine.Rows.scan_first_seen(
                    ctx, probes_dev, targets, self.mismatches, self.lcf_thres,
                    self.island_of_exact_match, 0, engine.SCAN_AUTO, order)
                first_universe, first_key = rows.first_seen_per_set(len(strs))
                rows.close()
            finally:
                targets.close()
        finally:
            probes_dev.close()
        seen = np.flatnonzero(first_universe >= 0)
        return seen[np.lexsort((first_key[seen], first_universe[seen]))].tolist()

    def ordered_probe_map_counts(self):
        """[(probe, sequences it maps to)] in the reference's order."""
        order = self._map_count_order()
        if self.either_strand:      # a probe stands where its first orientation is met
            order = list(dict.fromkeys(a % len(self.probes) for a in order))
        return [(self.probes[pi], self.probe_map_counts[self.probes[pi]]) for pi in order]

    def write_probe_map_counts(self, fn):
        write_probe_map_counts(self.ordered_probe_map_counts(), fn)


def add_uncovered_arguments(parser):
    """The options of the uncovered-region read-out, shared by the command lines."""
    parser.add_argument("--write-uncovered-regions",
                        help="TSV of the regions the probes leave uncovered: maximal runs of "
                             "bases, inside one sequence, below --uncovered-min-depth")
    parser.add_argument("--write-uncovered-fasta",
                        help="the uncovered regions of the forward strand as FASTA records")
    parser.add_argument("--uncovered-min-depth", type=int, default=1,
                        help="a base is uncovered when fewer than this many cover ranges hold it (default 1)")
    parser.add_argument("--uncovered-min-length", type=int, default=1,
                        help="report only regions of at least this many bases (default 1)")
    parser.add_argument("--uncovered-keep-ambiguous", action="store_true",
                        help="also report regions without a single A, C, G or T")


def uncovered_filters(args):
    """(min_depth, min_length, min_unambig) of the parsed options."""
    if args.uncovered_min_depth < 1 or args.uncovered_min_length < 1:
        raise ValueError("--uncovered-min-depth and --uncovered-min-length must be at least 1")
    return (args.uncovered_min_depth, args.uncovered_min_length, 0 if args.uncovered_keep_ambiguous else 1)


def write_uncovered(analyzer, args):
    """--write-uncovered-regions / --write-uncovered-fasta of one analyzer that has run."""
    if not (args.write_uncovered_regions or args.write_uncovered_fasta):
        return
    filters = uncovered_filters(args)
    if args.write_uncovered_regions:
        analyzer.write_uncovered_regions(args.write_uncovered_regions, *filters)
    if args.write_uncovered_fasta:
        analyzer.write_uncovered_fasta(args.write_uncovered_fasta, *filters)
    analyzer.log_uncovered_summary("", *filters)


def write_probe_map_counts(probe_map_counts, fn):
    """probe_map_counts: (probe, count) pairs."""
    with open(fn, "w") as f:
        f.write("\t".join(["Probe identifier", "Probe sequence",
                           "Number sequences mapped to"]) + "\n")
        for p, count in probe_map_counts:
            ident = p.identifier() if hasattr(p, "identifier") else ""
            f.write("\t".join(str(x) for x in [ident, p.seq_str, count]) + "\n")


def print_table(data):
    """The report's table as the reference prints it (:531-533): its table
    string ends in a newline, so print() leaves an empty line after it."""
    print(_table(data, ["left", "right", "right"]) + "\n")


def _table(data, col_justify):
    """Plain-text table with multi-line cells and an underlined header
    (layout of catch/utils/pretty_print.py:7-90)."""
    cells = [[str(c).rstrip().split("\n") for c in row] for row in data]
    widths = [max(len(line) for row in cells for line in row[j])
              for j in range(len(data[0]))]
    out = []
    for r, row in enumerate(cells):
        height = max(len(c) for c in row)
        for h in range(height):
            parts = []
            for j, c in enumerate(row):
                text = c[h] if h < len(c) else ""
                if col_justify[j] == "right":
                    parts.append(text.rjust(widths[j]))
                elif col_justify[j] == "center":
                    parts.append(text.center(widths[j]))
                else:
                    parts.append(text.ljust(widths[j]))
            out.append(" ".join(parts).rstrip())
        if r == 0:
            out.append(" ".join("-" * w for w in widths))
    return "\n".join(out)
