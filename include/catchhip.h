/*
 * catchhip.h -- C ABI of libcatchhip.so: the MI355X (gfx950) implementation of
 * the probe-coverage / set-cover / near-duplicate hot path of
 * broadinstitute/catch v1.5.2.
 *
 * The reference is pure Python and has no FFI of its own: the functions below
 * are what a ctypes binding for this path binds (INTEGRATION.md shows the
 * stub).  Each entry point cites the reference code (relative to the
 * reference repository root) whose behaviour it replaces.  Plain pointers and
 * sizes only; every buffer named `const T* x` is a caller-owned HOST buffer
 * unless the comment says "device".  All functions return 0 on success and a
 * negative CATCHHIP_E* code on failure; catchhip_last_error() gives the
 * message for the calling thread.  One host thread per context.
 * Two entry points build set cover instances the reference cannot state
 * (catchhip_rows_subtract: beside probes owned already;
 * catchhip_rows_below_depth: one layer of a design that covers every base
 * several times); the solvers they feed are the reference's.  A third,
 * catchhip_rows_prune, takes picks away again: those that cover nothing alone.
 * A fourth, catchhip_rows_pick_gains, reports what each pick added when it was
 * taken and the coverage after the first k picks (designs under a probe budget).
 *
 * Coordinates.  A `targets` object is a list of sequences, concatenated in
 * the order given; consecutive sequences with the same genome index form one
 * genome (= one "universe" of the set cover, catch/filter/
 * set_cover_filter.py:414-453).  Cover rows are reported in genome
 * coordinates (position within the genome's concatenated sequences), exactly
 * as SetCoverFilter._make_sets builds them.
 */
#ifndef CATCHHIP_H
#define CATCHHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CATCHHIP_ABI_VERSION 2

#define CATCHHIP_OK 0
#define CATCHHIP_EINVAL (-1)   /* bad argument */
#define CATCHHIP_EHIP (-2)     /* HIP runtime error */
#define CATCHHIP_ENOMEM (-3)   /* allocation failed */
#define CATCHHIP_ERANK (-4)    /* rank list exhausted (reference: IndexError) */
#define CATCHHIP_ECOMM (-5)    /* RCCL error */

typedef struct catchhip_ctx catchhip_ctx;
typedef struct catchhip_targets catchhip_targets;
typedef struct catchhip_probes catchhip_probes;
typedef struct catchhip_rows catchhip_rows;

int catchhip_abi_version(void);
/* The message of the calling thread's last failing call.  It is thread-local;
 * EVERY call that returns a non-zero code sets it before it returns, so the
 * text read right after a failure belongs to that failure and never to an
 * earlier call (a successful call leaves it alone: read it only after a
 * non-zero return).  For CATCHHIP_EHIP it names the failing HIP call with its
 * source line and hipGetErrorString of the error that call returned; for
 * CATCHHIP_EINVAL it says which argument or input was refused.  A call that
 * fails hands out no object and has returned every device block it took. */
const char *catchhip_last_error(void);

/* ---- context: one HIP device + one stream ----------------------------- */
int catchhip_device_count(int *count);
int catchhip_ctx_create(int device, catchhip_ctx **out);
int catchhip_ctx_destroy(catchhip_ctx *ctx);
int catchhip_ctx_sync(catchhip_ctx *ctx);
/* Device-memory cache of the library (all contexts): out4 = {hipMalloc calls so
 * far, bytes held from the driver, bytes of those currently free in the cache,
 * hipMalloc failures answered by emptying the caller's cache}.  No reference
 * counterpart (the reference keeps its working set in Python objects); the bench
 * reports it so that a step that allocates is visible. */
int catchhip_pool_stats(int64_t *out4);
/* Returns every idle cached block of every context of the process to the driver, after a synchronisation of
 * the current device (blocks of other devices: hipFree itself waits for the device that owns the block).  For the seams of a long-running process whose next
 * phase allocates differently (the cache is keyed by context and size class). */
int catchhip_pool_trim(void);
/* Elapsed GPU milliseconds spent in the kernels of the most recent call of
 * the named phase (HIP events on the context's stream).  phase: 0 = cover
 * scan kernels (K1 hit search), 1 = row build (sort/merge), 2 = greedy
 * set-cover kernels (set-up + solver), 3 = near-duplicate kernels, 4 = only the
 * (count+claim, check+apply) launch pairs of the frontier solver's rounds,
 * 5 = only the seed-verify launch of the seed scan (part of phase 0),
 * 6 = only the claim launches of the row-parallel solver (part of phase 4;
 * 0 launches when the last solve used the other kernels), 7 = only the
 * counting pass of the key-grouped join (part of phase 0; 5 is its writing
 * pass), 8 = the launches of
 * catchhip_pool_solve (one per dataset + the walk back), 9 = the flag kernel of
 * the last candidate pre-filter (catchhip_candidates_drop_polya,
 * catchhip_candidates_drop_composition, catchhip_candidates_drop_structure,
 * catchhip_candidates_drop_tm or catchhip_candidates_drop_background; the
 * compaction after it is not in it), or the build of the last
 * catchhip_kmer_index_create.
 * *launches = kernel launches timed. */
int catchhip_ctx_last_kernel_ms(catchhip_ctx *ctx, int phase, double *ms,
                                int64_t *launches);
/* Work counters of the most recent calls (for roofline accounting), 8 values:
 * [0] raw hits found by the last cover scan, [1] seeds verified (seed scan /
 * seed join), [2] greedy iterations (rounds), [3] picks, [4] winner rows applied
 * (sequential solver; row-parallel solver: row records streamed), [5] rows
 * re-counted by the greedy solver, [6] bitmap
 * words read while re-counting, [7] cover rows of the last fused
 * catchhip_setcover_filter call. */
int catchhip_ctx_last_counters(catchhip_ctx *ctx, int64_t *out8);
/* Work of the last key-grouped join (the seed scan of pigeonhole tables, csrc/scan_join.inc): out4[0] = target
 * positions whose k-mer is in the anchor table, [1] = (position, entry) pairs verified (the table matches of
 * catch/probe.py:1062-1069), [2] = lane slots the wave-wide runs occupied (64 per window chunk and entry; pairs /
 * slots = lane utilisation), [3] = tasks of runs that were cut by entries.  Zeros after a seed-list scan. */
int catchhip_ctx_last_join_counters(catchhip_ctx *ctx, int64_t *out4);
/* Capacity events of the last cover scan (catchhip_cover_scan and its kin, catchhip_tolerant_bp, the scan inside
 * catchhip_setcover_filter) or near-duplicate filter (catchhip_ndf_*, catchhip_candidates_ndf_*) on this context;
 * each of these calls zeroes all eight on entry (catchhip_setcover_grid: those of its last scan).  Many device
 * buffers are sized by an estimate: a kernel counts past the capacity without writing past it, the host reads the
 * count and runs again at the exact size, or takes a slower exact path.  out8[i] = how often that happened:
 * [0] the seed-list scan's work list, [1] the work list of the general scan's table look-up, [2] the general scan's
 * join of byte hashes, [3] the tiled scan's hit list, [4] the general scan's list of cut windows (every seed was then
 * extended by bytes), [5] the key-grouped join's list of tasks of cut runs (the seed-list scan ran instead),
 * [6] the edge list of a near-duplicate filter, [7] spare (0).  Results never depend on them. */
int catchhip_ctx_last_capacity_events(catchhip_ctx *ctx, int64_t *out8);

/* Of counter [1] (entries of the last seed scan's work list): those the
 * look-up's anchor-pair filter left without a seed -- a lower anchor of the same
 * probe is exact at the same window (the pair is reported from that anchor's
 * seed), or no second anchor of the probe matches (more than m mismatches).
 * They cost the verification 4 bytes each and none of its gathers. */
int catchhip_ctx_last_seeds_dropped(catchhip_ctx *ctx, int64_t *out);
/* 1 when the last catchhip_setcover_filter on this context solved from the row
 * build's bucketed records (no SoA row table was written), 0 otherwise. */
int catchhip_ctx_last_rows_direct(catchhip_ctx *ctx, int64_t *out);
/* Work of the row-parallel frontier solver in the last solve that used it (zeros
 * otherwise), 4 values: row records streamed by the count launches (alive rows,
 * summed over the rounds); of those, rows whose bitmap words were read again
 * because one of them had changed (SURVEY 8(d) K2's E_dirty -- the reference's
 * memo invalidation by overlap, catch/utils/set_cover.py:552-613, is the same
 * idea); bitmap words read for them; owner words the claim launches looked at. */
int catchhip_ctx_last_solver_counters(catchhip_ctx *ctx, int64_t *out4);
/* Gain bands of the last solve by the row-parallel solver (zeros otherwise), 2
 * values: the levels it went through (1: every row was awake from the first
 * round on) and the bands its sets were cut into. */
int catchhip_ctx_last_solver_levels(catchhip_ctx *ctx, int64_t *out2);
/* Of the same solve: the groups whose sets were cut into bands by boundaries of
 * their own (rows of a scan with group numbers, more than one band); 1 when
 * one row of boundaries served every set, 0 when the solver did not run. */
int catchhip_ctx_last_solver_band_groups(catchhip_ctx *ctx, int64_t *out1);
/* Work of the last Hamming near-duplicate filter on this context (SURVEY 8(d)
 * K3's quantities; catch/filter/near_duplicate_filter.py:47-142 does the same
 * look-ups probe by probe): probes N, tables T, pairs sharing a bucket that were
 * compared (C, all tables), pairs within the distance (edges). */
int catchhip_ctx_last_ndf_counters(catchhip_ctx *ctx, int64_t *out4);

/* ---- inputs ------------------------------------------------------------ */
/* Target sequences (catch/genome.py Genome.seqs of every genome of a group).
 * bytes: concatenation of the nseq sequences (raw characters, compared by
 * equality exactly as the reference compares str characters);
 * seq_off[nseq+1]; seq_genome[nseq] non-decreasing genome index in
 * [0, ngenomes). Uploads and bit-packs on the device. */
int catchhip_targets_create(catchhip_ctx *ctx, const uint8_t *bytes,
                            const int64_t *seq_off, const int32_t *seq_genome,
                            int64_t nseq, int32_t ngenomes,
                            catchhip_targets **out);
/* The same targets from one pointer per sequence (seq_ptr[i], seq_len[i] bytes
 * each; what a host that keeps its sequences as separate strings has): the
 * library gathers them into pinned memory with a few threads and uploads from
 * there, instead of the caller concatenating them first. */
int catchhip_targets_create_ptrs(catchhip_ctx *ctx, const uint8_t *const *seq_ptr,
                                 const int64_t *seq_len, const int32_t *seq_genome,
                                 int64_t nseq, int32_t ngenomes,
                                 catchhip_targets **out);
int catchhip_targets_destroy(catchhip_targets *t);
/* Hand-over of an input object to another context of the same device.  The
 * reference overlaps nothing here (catch/filter/set_cover_filter.py:816-846
 * builds a group's sets, then solves it); this path packs and uploads group
 * i + 1 on an upload context while the compute context scans and solves group
 * i, and the finished object changes hands: the call waits for the stream the
 * object was built on, after which only calls on `to` may use it. */
int catchhip_targets_rebind(catchhip_targets *t, catchhip_ctx *to);

/* Candidate probes + their seed ("anchor") table, i.e. the content of the
 * reference's kmer_probe_map (catch/probe.py:507-577 builds it,
 * :580-763 stores it): nprobes UNIQUE probe sequences (bytes/probe_off),
 * set_id[nprobes] = the set-cover set id that owns each unique probe
 * (catch/filter/set_cover_filter.py:408-412), and nent unique
 * (ent_probe, ent_pos) anchors of common length k. */
int catchhip_probes_create(catchhip_ctx *ctx, const uint8_t *bytes,
                           const int64_t *probe_off, int64_t nprobes,
                           const int32_t *set_id, const int32_t *ent_probe,
                           const int32_t *ent_pos, int64_t nent, int32_t k,
                           catchhip_probes **out);
int catchhip_probes_destroy(catchhip_probes *p);
int catchhip_probes_rebind(catchhip_probes *p, catchhip_ctx *to);   /* see catchhip_targets_rebind */

/* ---- K1: coverage scan -------------------------------------------------- */
#define CATCHHIP_SCAN_AUTO 0     /* seed scan when its preconditions hold, else general */
#define CATCHHIP_SCAN_GENERAL 1  /* force the seed-join + extension path */
#define CATCHHIP_SCAN_FAST 2     /* force the tiled Hamming kernel: the seed
                                    kernel's conditions + pigeonhole anchors
                                    {0,k,..,L-k} with L/k > mismatches (EINVAL
                                    otherwise) */
#define CATCHHIP_SCAN_SEED 3     /* force the hash-seeded Hamming kernel: equal-
                                    length DNA probes, lcf_thres == probe length,
                                    island == 0, sequences >= probe length; any
                                    anchor table (EINVAL otherwise) */
/* Replaces SetCoverFilter._make_sets (catch/filter/set_cover_filter.py
 * :359-470) = for every target sequence, probe.find_probe_covers_in_sequence
 * (catch/probe.py:1008-1271) under the default hybridization model
 * probe_covers_sequence_by_longest_common_substring(mismatches, lcf_thres,
 * island) (catch/probe.py:1274-1346, catch/utils/longest_common_substring.py
 * :59-159), then cover_extension / clip / genome offset (:424-453) and
 * IntervalSet normalisation (catch/utils/interval.py:25-44, :288-316).
 * Result: device-resident rows (set id, universe, start, end) sorted by
 * (set id, universe, start); *nrows = number of rows. */
int catchhip_cover_scan(catchhip_ctx *ctx, const catchhip_probes *probes,
                        const catchhip_targets *targets, int32_t mismatches,
                        int32_t lcf_thres, int32_t island,
                        int32_t cover_extension, int32_t mode,
                        catchhip_rows **out, int64_t *nrows);
/* The same scan without the interval merge: what coverage_analysis.Analyzer
 * ._find_covers_in_target_genomes collects (catch/coverage_analysis.py
 * :183-280) = for every sequence probe.find_probe_covers_in_sequence(
 * merge_overlapping=False) (catch/probe.py:1263-1270: duplicate ranges of a
 * probe removed, nothing merged), every range extended by cover_extension and
 * clipped to its sequence.  Rows (set id, universe, start, end) sorted by (set
 * id, start, end) in genome coordinates; pass one genome per sequence to keep
 * sequences apart.  EINVAL if one probe has more than 8192 ranges. */
int catchhip_cover_ranges(catchhip_ctx *ctx, const catchhip_probes *probes,
                          const catchhip_targets *targets, int32_t mismatches,
                          int32_t lcf_thres, int32_t island,
                          int32_t cover_extension, int32_t mode,
                          catchhip_rows **out, int64_t *nrows);
/* Copy rows to the host (arrays of length nrows). */
int catchhip_rows_fetch(catchhip_ctx *ctx, const catchhip_rows *rows,
                        int32_t *set_id, int32_t *universe, int64_t *start,
                        int64_t *end);
/* Build a rows object from host arrays (sorted by (set, universe, start),
 * disjoint non-touching within (set, universe)); genome_len[ngenomes] gives
 * the coordinate range of each universe.  Lets the greedy solver run on
 * externally supplied instances (the reference's set_cover unit tests). */
int catchhip_rows_from_host(catchhip_ctx *ctx, const int32_t *set_id,
                            const int32_t *universe, const int64_t *start,
                            const int64_t *end, int64_t nrows,
                            const int64_t *genome_len, int32_t ngenomes,
                            catchhip_rows **out);
int catchhip_rows_destroy(catchhip_rows *r);

/* Replaces SetCoverFilter._compute_tolerant_bp_covered_within_sequence
 * (catch/filter/set_cover_filter.py:472-529) for every sequence of
 * `targets` (the caller adds reverse-complement sequences to `targets`):
 * bp_out[i] += sum over sequences of the total length of the merged cover
 * ranges of unique probe i (bp_out has nprobes entries, host). */
int catchhip_tolerant_bp(catchhip_ctx *ctx, const catchhip_probes *probes,
                         const catchhip_targets *targets, int32_t mismatches,
                         int32_t lcf_thres, int32_t island, int64_t *bp_out);

/* ---- K2: greedy multi-universe set cover ------------------------------- */
/* Replaces set_cover.approx_multiuniverse(sets, costs == 1, universe_p,
 * ranks, use_intervalsets=True) (catch/utils/set_cover.py:147-615) as called
 * by catch/filter/set_cover_filter.py:113-144.  num_sets = number of
 * candidate probes (set ids 0..num_sets-1); ranks[num_sets] (NULL = all
 * equal); universe_p[ngenomes] float64 coverage fraction per universe
 * (NULL = 1.0).  out_ids (capacity num_sets) receives the chosen set ids,
 * *n_out their number, in the order in which the sequential algorithm picks
 * them (the reference returns a Python set; the order is the one of its loop).
 * When every universe_p is 1 and rows are at most 257 elements the solver takes
 * all locally-maximal sets per round (setcover_batched.inc) and restores that
 * order by sorting on the accept-time key; otherwise it picks one set per
 * iteration. */
int catchhip_setcover_greedy(catchhip_ctx *ctx, const catchhip_rows *rows,
                             int64_t num_sets, const int64_t *ranks,
                             const double *universe_p, int64_t *out_ids,
                             int64_t *n_out);

/* Replaces SetCoverFilter._filter's device work for one group in ONE call
 * (catch/filter/set_cover_filter.py:816-846 = _make_sets then
 * set_cover.approx_multiuniverse): catchhip_cover_scan + catchhip_setcover_
 * greedy with the rows never leaving the device.  Arguments as for those two
 * functions; *nrows (may be NULL) receives the number of cover rows. */
int catchhip_setcover_filter(catchhip_ctx *ctx, const catchhip_probes *probes,
                             const catchhip_targets *targets,
                             int32_t mismatches, int32_t lcf_thres,
                             int32_t island, int32_t cover_extension,
                             int32_t mode, int64_t num_sets,
                             const int64_t *ranks, const double *universe_p,
                             int64_t *out_ids, int64_t *n_out, int64_t *nrows);
/* The same for n independent groups at once (the reference handles the groups
 * of a design one after the other, set_cover_filter.py:816-846 per group):
 * group g runs on ctxs[g] -- its own HIP stream -- driven by its own host
 * thread, so the groups' kernels overlap on the device.  All arrays have n
 * entries; ranks[g] / universe_p[g] may be NULL, as may the two arrays
 * themselves; out_ids[g] has room for num_sets[g] ids.  Contexts must be
 * distinct.  Returns the first failing group's error code (its message through
 * catchhip_last_error of the calling thread). */
int catchhip_setcover_filter_many(int32_t n, catchhip_ctx *const *ctxs,
                                  const catchhip_probes *const *probes,
                                  const catchhip_targets *const *targets,
                                  int32_t mismatches, int32_t lcf_thres,
                                  int32_t island, int32_t cover_extension,
                                  int32_t mode, const int64_t *num_sets,
                                  const int64_t *const *ranks,
                                  const double *const *universe_p,
                                  int64_t *const *out_ids, int64_t *n_out,
                                  int64_t *nrows);

/* ---- grid design: several cover extensions from one scan ----------------
 * Replaces the cover extension of SetCoverFilter._make_sets
 * (catch/filter/set_cover_filter.py:424-453 + catch/utils/interval.py
 * :288-316: every cover range extended by e, clipped to its sequence, the
 * ranges of a (set, universe) normalised) for n_ext values of e at once, from
 * the rows of ONE catchhip_cover_scan made with cover_extension = 0: row [s, t)
 * becomes [max(seqstart(s), s - e), min(seqend(t - 1), t + e)) and rows that
 * then overlap or touch merge.  The reference has no counterpart: it runs its
 * scan again for every e (README option #3 runs design.py once per grid point).
 * out[n_ext] receives n_ext row objects (for catchhip_setcover_greedy,
 * catchhip_rows_fetch, catchhip_rows_destroy), equal row for row to a scan at
 * that e, and nrows[n_ext] (may be NULL) their row counts.  CATCHHIP_EINVAL for a negative e, rows0 not from a cover scan at
 * e = 0, rows of a scan with group numbers (a union), or other targets. */
int catchhip_rows_extend(catchhip_ctx *ctx, const catchhip_rows *rows0,
                         const catchhip_targets *targets, int32_t n_ext,
                         const int32_t *ext, catchhip_rows **out,
                         int64_t *nrows);
/* gain0 of a rows object (per set id, the total length of its rows: the first
 * round's gains of a full-coverage solve; setcover_flat.inc reads it instead
 * of counting): copies min(n, *n_out) entries; *n_out = entries held (0: none).
 * No reference counterpart (the reference counts every round). */
int catchhip_rows_fetch_gain0(catchhip_ctx *ctx, const catchhip_rows *rows,
                              int64_t n, uint32_t *gain0, int64_t *n_out);
/* ---- extending an existing probe set: rows minus what is covered already ---
 * out = every maximal run of bases of every row of `rows` that no row of
 * `covered` touches, with the row's set and universe, in the order of `rows`:
 * the reduced set cover instance in which the sets behind `covered` count as
 * picked before the first round of catch/utils/set_cover.py:362-550 (their
 * elements leave every universe and every other set).  The reference has no
 * counterpart.  `rows`: a row table in the solver's form (a merged cover scan,
 * rows_from_host, rows_extend); `covered`: any row table over the same
 * coordinate space (equal universe lengths), any set ids, rows may overlap
 * across sets.  The result is sorted and normalised like `rows` (pieces of a
 * row are at least one covered base apart) and carries gain0 when `rows`
 * does; *nrows (may be NULL) = its row count.  An empty `covered` gives a copy
 * of `rows`.  CATCHHIP_EINVAL for deferred, direct or grouped rows (either
 * table), another coordinate space, or 2^32 - 1 target bases and more. */
int catchhip_rows_subtract(catchhip_ctx *ctx, const catchhip_rows *rows,
                           const catchhip_rows *covered,
                           catchhip_rows **out, int64_t *nrows);
/* ---- either strand: the union of two row tables, set by set -----------------
 * out = for every (set, universe) the normal form of the union of that pair's
 * rows in `a` and in `b`: rows that overlap or touch merge, rows of different
 * universes never do (not even where the last base of one universe and the
 * first of the next are neighbours in global coordinates).  It is the cover
 * set of a candidate that covers what its own string or another one -- its
 * reverse complement -- hybridises to (SetCoverFilter(either_strand=True)); the
 * reference looks at reverse complements for its ranks only
 * (catch/filter/set_cover_filter.py:472-529) and has no counterpart.  `a`, `b`:
 * row tables in the solver's form (a merged cover scan, rows_from_host,
 * rows_extend, the result of rows_subtract / rows_restrict) over the same
 * coordinate space (equal universe lengths); set ids are any non-negative
 * values, a set may have rows in one table only.  The result is sorted by
 * (set, universe, start), carries its exact longest row and -- when both
 * tables carry gain0 -- gain0 summed from its own rows, sized to the larger of
 * the two: it goes to catchhip_setcover_greedy as it is.  *nrows (may be NULL)
 * = its row count.  One table empty gives a copy of the other.
 * CATCHHIP_EINVAL for deferred, direct or grouped rows (either table), another
 * coordinate space, 2^32 - 1 target bases and more, 2^31 rows and more, or a
 * table found not to be in the solver's form.  Scratch: 16 bytes per input
 * row.  Timed as phase 1. */
int catchhip_rows_union(catchhip_ctx *ctx, const catchhip_rows *a,
                        const catchhip_rows *b, catchhip_rows **out,
                        int64_t *nrows);
/* *longest = the length of the longest row as the table holds it on the host
 * (the solvers size their tiles by it): exact for rows_from_host, rows_union,
 * rows_subtract, rows_restrict and rows_below_depth, 0 for an empty table.  No
 * device work.  CATCHHIP_EINVAL for deferred rows (the scan has not reported
 * yet). */
int catchhip_rows_longest(const catchhip_rows *rows, uint32_t *longest);
/* ---- coverage depth: rows below depth k under the picks so far --------------
 * out = every row of `rows` whose set is not in picks[0..npicks), cut into its
 * maximal runs of bases b with depth(b) < depth, where depth(b) = the number of
 * picked sets with a row over b (distinct sets: the rows of a set do not
 * overlap); set, universe and order kept.  It is the instance of layer `depth`
 * of a layered greedy that covers every base `depth` times: the sets picked by
 * the earlier layers are absent, and a base they cover `depth` times already has
 * left every universe and every other set.  The reference has no counterpart.
 * `rows`: a row table in the solver's form with set ids in [0, num_sets) (a
 * merged cover scan, rows_from_host, rows_extend).  The result is sorted and
 * normalised like `rows` (pieces of a row are at least one base apart),
 * carries gain0 when `rows` does and its exact longest row: it goes to
 * catchhip_setcover_greedy as it is.  *nrows (may be NULL) = its row count;
 * reached[u] (ngenomes values, may be NULL) = the bases of universe u with
 * depth(b) >= depth.  npicks == 0 gives a copy of `rows`, every set picked an
 * empty table.  CATCHHIP_EINVAL for depth < 1, a pick outside [0, num_sets) or
 * given twice, deferred, direct or grouped rows, 2^32 - 1 target bases and
 * more, 2^31 rows or pieces and more.  Scratch: 4 bytes + 1 bit per target
 * base.  Timed as phase 1. */
int catchhip_rows_below_depth(catchhip_ctx *ctx, const catchhip_rows *rows,
                              int64_t num_sets, const int64_t *picks,
                              int64_t npicks, int32_t depth,
                              catchhip_rows **out, int64_t *nrows,
                              int64_t *reached);
/* ---- pruning: the picks that cover nothing alone ---------------------------
 * Which of picks[0..npicks) (set ids in pick order) can leave without any base
 * falling below `depth`?  depth(b) = the picked sets with a row of `rows` over
 * b plus the rows of `fixed` over b (`fixed`: NULL, or any row table over the
 * same coordinate space -- probes that stay whatever happens; every one of its
 * rows counts).  The picks are examined from the last picked to the first; a
 * pick is removed if at its turn every base of every one of its rows has
 * depth >= depth + 1, and its removal lowers the depth of its bases by 1
 * before the next pick is examined.  min(depth(b), depth) is the same before
 * and after for every base, and no pick that stays is removable afterwards.
 * The device reproduces this walk exactly, in parallel rounds, with integer
 * arithmetic only: the result does not depend on launch geometry or on the
 * order of atomics.  removed_flags[i] (npicks bytes) = 1 if picks[i] was
 * removed; *nremoved their number; *rounds the rounds the device took (a
 * final one-workgroup walk counts as one).  The latter two may be NULL.  A
 * pick without rows is removed.  The reference has no counterpart.  `rows`: a
 * row table in the solver's form with set ids in [0, num_sets).  npicks == 0
 * returns at once.  CATCHHIP_EINVAL as catchhip_rows_below_depth: depth < 1, a
 * pick outside [0, num_sets) or given twice, deferred, direct or grouped rows
 * (either table), 2^32 - 1 target bases and more; and for a `fixed` table of
 * another context or coordinate space.  Scratch: 12 bytes + 1 bit per target
 * base.  Timed as phase 1. */
int catchhip_rows_prune(catchhip_ctx *ctx, const catchhip_rows *rows,
                        const catchhip_rows *fixed, int64_t num_sets,
                        const int64_t *picks, int64_t npicks, int32_t depth,
                        uint8_t *removed_flags, int64_t *nremoved,
                        int64_t *rounds);
/* ---- gain per pick: the bases each pick covered first ------------------------
 * picks[0..npicks) are set ids in pick order; rank(i) = i.  first(b) = the
 * smallest rank among the picks whose set has a row of `rows` over base b
 * (none if no pick covers b).  gains[i] (npicks values) = the number of bases b
 * with first(b) == i: what the pick added when it was taken.  A pick without
 * rows, or one wholly shadowed by earlier picks, gets 0.  At full coverage
 * without ranks these are the gains the greedy solver chose by, which it keeps
 * on the device.  checkpoints[0..ncheck) are pick counts k in [1, npicks],
 * strictly ascending.  For checkpoint k and universe u, cov_u(k) = covered0[u]
 * + the bases b of u with first(b) < k (covered0 == NULL: zeros).
 * covered_total[j] = the sum of cov_u(k_j) over the universes;
 * worst_universe[j] = the universe with denom[u] > 0 whose cov_u / denom[u] is
 * smallest, compared exactly by 64-bit cross-multiplication, ties to the lower
 * universe, -1 if no universe has a positive denominator; worst_covered[j] =
 * its cov_u (0 with -1).  With ncheck == 0 the six checkpoint and universe
 * arguments may be NULL.  All arithmetic is integer; the result depends neither
 * on launch geometry nor on the order of atomics.  The reference has no
 * counterpart.  `rows`: a row table in the solver's form with set ids in
 * [0, num_sets).  npicks == 0 returns at once and requires ncheck == 0.
 * CATCHHIP_EINVAL for a pick outside [0, num_sets) or given twice, deferred,
 * direct or grouped rows, 2^32 - 1 target bases and more, checkpoints out of
 * range or not strictly ascending, a denom[u] or covered0[u] + universe length
 * outside 32 bits, and ncheck x universes >= 2^31 (the caller splits the
 * checkpoints).  Any table below 2^31 rows is served: the kernels that take a
 * wavefront per row compute the row number in 64 bits.  Scratch: 4 bytes per
 * target base + 4 bytes x ncheck x universes.  Timed as phase 1. */
int catchhip_rows_pick_gains(catchhip_ctx *ctx, const catchhip_rows *rows,
                             int64_t num_sets, const int64_t *picks,
                             int64_t npicks, uint32_t *gains,
                             const int64_t *checkpoints, int64_t ncheck,
                             const int64_t *denom, const int64_t *covered0,
                             uint64_t *covered_total, int32_t *worst_universe,
                             int64_t *worst_covered);
/* One (probes, targets, mismatches) instance over n_ext cover extensions: the
 * reference's design.py run once per e (set_cover_filter.py:816-846 each time).
 * Scans once at e = 0, derives the rows at each ext[i] (catchhip_rows_extend,
 * one table at a time, the rows never leave the device) and solves each with
 * ranks / universe_p as catchhip_setcover_greedy: out_ids[i] (room for
 * num_sets ids), n_out[i], nrows[i] (may be NULL) per extension.  Test hook
 * CATCHHIP_GRID_RESCAN=1 scans afresh at each e instead. */
int catchhip_setcover_grid(catchhip_ctx *ctx, const catchhip_probes *probes,
                           const catchhip_targets *targets, int32_t mismatches,
                           int32_t lcf_thres, int32_t island, int32_t mode,
                           int32_t n_ext, const int32_t *ext, int64_t num_sets,
                           const int64_t *ranks, const double *universe_p,
                           int64_t *const *out_ids, int64_t *n_out,
                           int64_t *nrows);
/* Work of the last catchhip_setcover_grid on this context, 4 values: cover
 * scans, derived row tables, solves, rows of the e = 0 scan. */
int catchhip_ctx_last_grid_counters(catchhip_ctx *ctx, int64_t *out4);

/* ---- pooling: one designed grid point per dataset within a probe budget ----
 * Replaces param_search.standard_search / higher_dimensional_search +
 * _round_params (catch/pool/param_search.py:547-658, :661-749, :362-520; the
 * loss of :25-126 without its barrier term) as bin/pool.py calls them.  The
 * reference interpolates probe counts between grid points, minimises loss +
 * barrier from a random start and rounds; this is the exact minimum over the
 * designed points themselves (a multiple-choice knapsack).  Dataset i has
 * options opt_off[i] .. opt_off[i + 1] - 1 (opt_off[0] = 0) with counts[]
 * (probes) and losses[] (float64, finite), both host arrays of opt_off[D]
 * entries.  f_0[b] = 0 for 0 <= b <= budget; f_i[b] = min over options k with
 * count <= b of f_{i-1}[b - count] + loss, in float64, +inf where none fits,
 * the smallest k among equal values; the walk back from f_D[budget] gives
 * out_choice[D] (option index within its dataset), *out_total (sum of the
 * chosen counts) and *out_loss (= f_D[budget]: the chosen losses added in
 * dataset order).  One kernel launch per dataset, one lane per budget cell; the
 * D x (budget + 1) table of 16-bit choices stays on the device.
 * CATCHHIP_EINVAL with a message: the budget is below the sum of each dataset's
 * smallest count (the message names that sum), a dataset has no or more than
 * 65,535 options, a negative count, a loss that is not finite, or a choice
 * table larger than the device-memory cache may hold. */
int catchhip_pool_solve(catchhip_ctx *ctx, int64_t D, const int64_t *opt_off,
                        const int64_t *counts, const double *losses,
                        int64_t budget, int32_t *out_choice, int64_t *out_total,
                        double *out_loss);

/* ---- design_naively: redundancy graph, naive pass, dominating set ----------
 * The reference's two legacy filters evaluate a pairwise predicate
 * are_redundant(a, b) over all n (n - 1) / 2 pairs of a probe list in Python
 * (catch/filter/naive_redundant_filter.py:46-77, catch/filter/
 * dominating_set_filter.py:62-91).  catchhip_redundancy_graph evaluates the
 * predicate for every pair on the device (csrc/redundant.hip) and keeps the
 * result as an opaque device-resident graph in CSR form: symmetric, no self
 * loops, every neighbour list ascending; *nedges (64-bit, may be NULL) counts
 * the directed edges, two per redundant pair.  n probes at bytes / off[n + 1]
 * (duplicates allowed; letters ACGTN; at most 256 bases each -- CATCHHIP_EINVAL
 * names the limit otherwise).
 *   kind 0: naive_redundant_filter.redundant_shift_and_mismatch_count(shift =
 *           p0, mismatch_thres = p1) (:80-143): redundant iff for some offset s
 *           in [-p0, p0] the overlapping parts differ in at most p1 places; an
 *           empty overlap has 0 mismatches (the quick loop, :112-137).
 *   kind 1: naive_redundant_filter.redundant_longest_common_substring(
 *           mismatches = p0, lcf_thres = p1, prune_with_heuristic_and_anchor =
 *           False) (:146-215): redundant iff longest_common_substring.k_lcf(a, b,
 *           p0)[0] >= p1 (catch/utils/longest_common_substring.py:11-56), i.e.
 *           on some diagonal a window of p1 positions has at most p0 mismatches.
 *           Characters compare by plain inequality: N equals N.  p1 <= 0 makes
 *           every pair redundant and is refused with CATCHHIP_EINVAL (the caller
 *           knows the answer).  The reference's randomised heuristic (the True
 *           branch) is not reproduced: the exact predicate runs for every pair.
 * catchhip_redundancy_fetch copies the graph out: ptr[n + 1], idx[nedges]. */
typedef struct catchhip_redgraph catchhip_redgraph;
int catchhip_redundancy_graph(catchhip_ctx *ctx, const uint8_t *bytes,
                              const int64_t *off, int64_t n, int32_t kind,
                              int32_t p0, int32_t p1, catchhip_redgraph **out,
                              int64_t *nedges);
int catchhip_redundancy_fetch(catchhip_ctx *ctx, const catchhip_redgraph *graph,
                              int64_t *ptr, uint32_t *idx);
int catchhip_redundancy_destroy(catchhip_redgraph *graph);
/* Replaces NaiveRedundantFilter._filter's double loop (catch/filter/
 * naive_redundant_filter.py:46-77): keep[i] (host, n bytes) = 1 iff no kept
 * probe with a smaller index is redundant to probe i -- the lexicographically
 * first maximal independent set of the graph.  Frontier rounds on the device (a
 * vertex is dropped once a smaller neighbour is kept, kept once all smaller
 * neighbours are dropped; one read-back per 8 rounds) and, when a round decides
 * few vertices (a chain of dependencies), one single-workgroup launch that walks
 * the rest in order.  The graph never leaves the device. */
int catchhip_redundancy_naive(catchhip_ctx *ctx, const catchhip_redgraph *graph,
                              uint8_t *keep);
/* The set cover instance DominatingSetFilter._filter hands to set_cover.approx
 * (catch/filter/dominating_set_filter.py:62-91, catch/utils/set_cover.py:14-144,
 * cost 1 and p = 1): set i = {i} + neighbours of i, as a rows object for
 * catchhip_setcover_greedy with num_sets = n and one universe in which element
 * u is the row [2 u, 2 u + 1).  approx picks the largest gain and, of equal
 * gains, the lowest id (it iterates a set of small dense ints), which is the
 * solver's order.  The probes of the graph must be distinct: approx's universe
 * holds Probe objects that hash by sequence, so the caller builds the graph on
 * first occurrences.  *nrows = nedges + n (fewer than 2^31, else EINVAL). */
int catchhip_redundancy_rows(catchhip_ctx *ctx, const catchhip_redgraph *graph,
                             catchhip_rows **out, int64_t *nrows);

/* Multi-GPU, one process per GPU: an RCCL communicator attached to a context
 * (the reference has no counterpart: it forks a process pool,
 * catch/probe.py:727-743, catch/filter/set_cover_filter.py:848-900).  The
 * communicator carries the exchanges of universe-sharded instances
 * (catchhip_shard_allreduce, catchhip_shard_solve); every other call on the
 * context runs as on any other context. */
int catchhip_comm_unique_id(uint8_t *id128);
int catchhip_comm_init(catchhip_ctx *ctx, const uint8_t *id128, int32_t nranks,
                       int32_t rank);
int catchhip_comm_destroy(catchhip_ctx *ctx);
/* Collective: every rank of the communicator fills nelem uint32 with rank + 1, SUM
 * all-reduces them on the context's stream and checks every element against
 * nranks (nranks + 1) / 2.  CATCHHIP_ECOMM with the RCCL error or the number of wrong
 * elements.  catch_amd.parallel.init_from_env runs it once after catchhip_comm_init and
 * falls back to the host exchange, by agreement of all ranks, if any rank fails. */
int catchhip_comm_selftest(catchhip_ctx *ctx, int64_t nelem);
/* Test entry points of the two device-wide primitives every kernel family builds
 * on (csrc/primitives.hip); tests/test_primitives.py compares them with NumPy.
 * No reference counterpart.
 * _scan_u32: out[i] = in[0] + .. + in[i-1] (mod 2^32) for n values; in_place != 0
 * scans the uploaded buffer onto itself, otherwise into a second buffer.
 * _sort_pairs: keys / vals hold n * max(nseg, 1) pairs and come back as the device
 * buffers stand after the call.  nseg == 0: one stable sort of n pairs on
 * max(1, ceil(key_bits / 8)) 8-bit digits from first_bit upwards; nseg >= 1:
 * nseg segments of n pairs side by side, each sorted on its own.  The sort's own
 * refusals (CATCHHIP_EINVAL) come back unchanged. */
int catchhip_selftest_scan_u32(catchhip_ctx *ctx, const uint32_t *in, int64_t n,
                               int32_t in_place, uint32_t *out);
int catchhip_selftest_sort_pairs(catchhip_ctx *ctx, uint64_t *keys, uint32_t *vals,
                                 int64_t n, int64_t nseg, int32_t key_bits,
                                 int32_t first_bit);
/* Test entry points of the wavefront-level helpers the kernels share (csrc/wave.h).
 * _wave: n words (a multiple of 256, at most 2^24), one 256-thread workgroup per 256,
 * one word per thread.  out32 holds 10 arrays of n words, [k * n + i] = what helper k
 * returned to thread i: 0 wave_sum, 1 wave_max, 2 wave_sum_all, 3 wave_max_all,
 * 4 wave_incl_scan, 5 wave_excl_scan, 6 its total, 7 wave_incl_scan_dpp, 8 quad_sum,
 * 9 row8_sum.  out64 holds 2 arrays of n: 0 wave_max, 1 wave_incl_scan of the 64-bit
 * value ((in[i] & 0xffff) << 32) | in[i].
 * _find_segment: out[j] = find_segment(off, n, x[j]) for nx values; off has n + 1
 * entries, off[0] = 0, non-decreasing; x[j] < off[n] is the caller's business. */
int catchhip_selftest_wave(catchhip_ctx *ctx, const uint32_t *in, int64_t n,
                           uint32_t *out32, uint64_t *out64);
int catchhip_selftest_find_segment(catchhip_ctx *ctx, const uint32_t *off, int64_t n,
                                   const uint32_t *x, int64_t nx, uint32_t *out);
/* Test entry point of the base-interval helpers of csrc/spans.h: n intervals [a[i], b[i]),
 * a[i] < b[i] <= 64 * nwords, one per thread, over the bitmap bm of nwords words.
 * out32 holds 4 arrays of n: 0 first word, 1 number of words, 2 span_popc, 3 span_all_set;
 * out64 holds 3 arrays of n: 0 mask of the first word, 1 of the last, 2 span_in_word for
 * word `view` (0 where the interval does not reach that word).  A second launch has all
 * threads span_paint into one zeroed bitmap (painted: nwords words) and span_mark_diff
 * into one zeroed difference array (diff: 64 * nwords + 1 words). */
int catchhip_selftest_spans(catchhip_ctx *ctx, const uint64_t *bm, int64_t nwords,
                            const uint32_t *a, const uint32_t *b, int64_t n, uint32_t view,
                            uint32_t *out32, uint64_t *out64, uint64_t *painted,
                            uint32_t *diff);
/* Test entry point of the bucketed row build (csrc/rows_bucket.inc and its host side
 * in csrc/scan.hip); tests/test_row_build.py compares it with a sequential merge in
 * NumPy.  No reference counterpart.  Hit records go in as a producer files them, the
 * build's own functions run as the scans call them, everything they leave comes out.
 * rec: nrec records of 4 words {start, end, segment, bucket}, nb buckets.  Producer:
 *  - scattered (bstart_in == NULL): rank[d] = arrival index of record d inside its
 *    bucket or 0xffffffff for a miss, bcnt[b] = hits of bucket b; with wcnt (one word
 *    per 64 records) only the first wcnt[d / 64] records of every 64 are looked at;
 *  - grouped (bstart_in: nb + 1 offsets): record i already stands at its place;
 *    run_cnt (or NULL) [b * run_stride + a] = length of sorted run a < nruns of bucket b.
 * bucket_set (or NULL): bucket -> set id.  bounds: nbounds + 1 segment offsets of the
 * start coordinates, needed by the radix build only.
 * opt: [0] dedupe (equal ranges collapse, nothing merges), [1] per-bucket sums wanted,
 * [2] 0 = bucketed build, 1 = radix build, 2 = radix build iff a bucket overflowed,
 * [3] emit 0 = with the counts known to the host, 1 = one slot per hit, counts read
 * on the device.  Scattered records only for [2] != 0.
 * Out: the table (o_set / o_seg / o_start / o_end, room for one row per hit), per
 * bucket o_mcnt / o_blmax / o_bsum (nb each; o_bsum only with opt[1]), o_bstart
 * (nb + 1), o_S = the grouped records after the merge (4 words per hit), scalars[5] =
 * hits, rows, longest row, overflow flag, radix build used.
 * CATCHHIP_EINVAL when a rank, a bucket or an offset would point outside its array. */
int catchhip_selftest_row_build(catchhip_ctx *ctx, const uint32_t *rec, const uint32_t *rank,
                                const uint32_t *wcnt, int64_t nrec, const uint32_t *bcnt,
                                const uint32_t *bstart_in, int64_t nb, const int32_t *bucket_set,
                                const uint32_t *run_cnt, int32_t run_stride, int32_t nruns,
                                const uint32_t *bounds, int64_t nbounds, const int32_t *opt,
                                int32_t *o_set, int32_t *o_seg, uint32_t *o_start,
                                uint32_t *o_end, uint32_t *o_mcnt, uint32_t *o_blmax,
                                uint64_t *o_bsum, uint32_t *o_S, uint32_t *o_bstart,
                                int64_t *scalars);
/* Test entry point of the seed table (the hash table of the anchor k-mers that both
 * seed scans look target k-mers up in; csrc/scan.hip); tests/test_seed_table.py
 * compares it with a dictionary built in NumPy.  No reference counterpart.  Builds the
 * table of P for `mismatches` as the key-grouped join does (as_list == 0) or as the
 * seed-list scan does (as_list != 0; allow_filter: its anchor-pair filter may apply)
 * and copies it out.  slot_room: slots the caller has room for -- o_slots 4 words per
 * slot {key lo, key hi, first, count}, o_present slot_room / 8 words; o_ents and
 * o_aslot one word per anchor entry of P (o_aslot is written only with the filter on).
 * scalars[8] = capacity (slots), slots with entries, set presence bits, presence
 * words (0: no presence filter), bits a key sets in its word, entries in the table,
 * filter on (0 / 1), anchors per probe (0: not a pigeonhole table).
 * CATCHHIP_EINVAL when the table does not fit slot_room. */
int catchhip_selftest_seed_table(catchhip_ctx *ctx, const catchhip_probes *P, int32_t mismatches,
                                 int32_t as_list, int32_t allow_filter, int64_t slot_room,
                                 uint32_t *o_slots, uint32_t *o_ents, uint32_t *o_present,
                                 uint32_t *o_aslot, int64_t *scalars);
/* Test entry point of the launch plans of the candidate rules (csrc/rule_host.h);
 * tests/test_candidate_launch_plan.py compares them with the tests' own arithmetic.
 * Host arithmetic only: no context, no device.  No reference counterpart.
 * Rows of L characters with row_extra bytes per row and wg_extra bytes per workgroup
 * behind them, the latter aligned to tail_align (4 or 8) bytes, aligned16 != 0: the
 * byte array is 16-byte aligned.  row_out[7] = rows per workgroup, staged (0 / 1),
 * 16-byte chunks per row, row pitch in dwords, dword offset of the per-row extras, of
 * the per-workgroup extras, bytes of dynamic LDS.
 * Planes of L characters with plane_tail bytes per workgroup behind them, aligned to
 * plane_align.  plane_out[5] = words per plane, candidates per workgroup, planes in
 * LDS (0 / 1), dword offset of the tail, bytes of dynamic LDS. */
int catchhip_selftest_candidate_plan(int32_t L, int64_t row_extra, int64_t wg_extra,
                                     int32_t tail_align, int32_t aligned16,
                                     int64_t plane_tail, int32_t plane_align,
                                     uint32_t *row_out, uint32_t *plane_out);
/* Which RCCL the communicators of this library go through: "RCCL version code V
 * from <file> (<how it was chosen>)".  The library opens ONE copy by path
 * (CATCHHIP_RCCL_PATH, else /opt/rocm/lib/librccl.so) instead of whatever file of
 * that soname the process mapped first (torch ships its own).  No reference
 * counterpart (the reference is single-process Python). */
int catchhip_comm_info(char *buf, int64_t len);

/* ONE set cover instance with its UNIVERSES (target genomes) sharded over
 * ranks -- set_cover.approx_multiuniverse (catch/utils/set_cover.py:147-615)
 * for a group too large for one GPU's share of the work.  Every rank scans
 * all candidate probes against its own contiguous range of the group's genomes
 * (catchhip_cover_scan on a targets object holding just those) and creates a
 * shard from its rows; num_sets and ranks are the same everywhere.  The
 * frontier solver then runs in rounds, each of which the caller drives:
 *     catchhip_shard_count        local gains           (enqueued)
 *     all-reduce SUM of the gain buffer   (catchhip_shard_allreduce(S, 0), or
 *                                          _allreduce_local for shards of one process)
 *     catchhip_shard_claim_check  claims + local losses (enqueued)
 *     all-reduce MAX of the lost buffer   (which = 1)
 *     catchhip_shard_apply        accepted sets applied; synchronises (the one
 *                                 host synchronisation of a round); *done =
 *                                 1 finished, -1 ranks exhausted, 0 next round
 * and catchhip_shard_picks returns the picks in the sequential pick order --
 * the same list on every rank, identical to the unsharded solver's.  A shard is
 * single-use: once it has reported done, the steps and catchhip_shard_solve
 * refuse it (CATCHHIP_EINVAL); only _picks, _info and _destroy remain.
 * Instances of 1 to 2^25 sets with rows of at most 257 bases, full or partial
 * coverage; anything else is refused with CATCHHIP_EINVAL ("... solved
 * unsharded") and solved whole on one rank (catch_amd/parallel.py).
 * Partial coverage (catchhip_shard_create_p with universe_p, one fraction per
 * LOCAL universe, some below 1; set_cover.py:362-373, 393-433): need[u] and the
 * acceptance thresholds of a universe live on the rank that owns it; a claimant
 * that lost nowhere must also pass the universe test on EVERY rank, so a round
 * has a third step between the lost exchange and the apply:
 *     catchhip_shard_verdict      local universe tests of the candidates left; a
 *                                 failure is one more lost mark (enqueued)
 *     all-reduce MAX of the lost buffer once more (which = 1)
 * (a no-op for shards created without universe_p).
 * catchhip_shard_buffers exposes the two exchange buffers (device pointers:
 * uint32[gain_count], uint8[lost_count]) for callers with their own
 * transport.  Ask again after EVERY apply: the buffers are packed -- only the
 * sets whose global gain was still positive at the last apply travel, in set
 * order, a list every rank derives from the same all-reduced gains (gain_count
 * = lost_count + 2) -- so the counts shrink from round to round (they are the
 * same on every rank) and may reach 0, in which case there is nothing to
 * exchange but the two extra gain slots. */
typedef struct catchhip_shard catchhip_shard;
int catchhip_shard_create(catchhip_ctx *ctx, const catchhip_rows *rows,
                          int64_t num_sets, const int64_t *ranks,
                          catchhip_shard **out);
int catchhip_shard_create_p(catchhip_ctx *ctx, const catchhip_rows *rows,
                            int64_t num_sets, const int64_t *ranks,
                            const double *universe_p, catchhip_shard **out);
/* instance_partial: 1 / 0 = whether any universe of the WHOLE instance (on any
 * rank) has a fraction below 1 -- the caller passes the same value on every
 * rank so that all of them run the same kernels and refuse the same instances
 * even when a rank's own universes all have fraction 1 (coverage given in
 * bases: catch/filter/set_cover_filter.py:761-792); -1 = decide from this
 * shard's universe_p (what catchhip_shard_create_p does). */
int catchhip_shard_create_pi(catchhip_ctx *ctx, const catchhip_rows *rows,
                             int64_t num_sets, const int64_t *ranks,
                             const double *universe_p, int instance_partial,
                             catchhip_shard **out);
int catchhip_shard_verdict(catchhip_shard *shard);
int catchhip_shard_destroy(catchhip_shard *shard);
int catchhip_shard_count(catchhip_shard *shard);
int catchhip_shard_claim_check(catchhip_shard *shard);
int catchhip_shard_apply(catchhip_shard *shard, int32_t *done);
int catchhip_shard_buffers(catchhip_shard *shard, void **gain,
                           int64_t *gain_count, void **lost,
                           int64_t *lost_count);
int catchhip_shard_picks(catchhip_shard *shard, int64_t *out_ids,
                         int64_t *n_out);
/* out4 = {elements of the gain buffer (uint32) and of the lost buffer (uint8)
 * in the NEXT exchange, bytes per lost element (1), 1 | 2 if the instance is
 * partial}. */
int catchhip_shard_info(catchhip_shard *shard, int64_t *out4);
/* which: 0 = gain buffer (SUM), 1 = lost buffer (MAX).  _allreduce uses the
 * context's RCCL communicator (stream-ordered); _allreduce_local reduces the
 * buffers of n <= 64 shards that live in this process on one device. */
int catchhip_shard_allreduce(catchhip_shard *shard, int32_t which);
/* Exchange buffer `which` to (to_host != 0) or from a host array of the
 * buffer's size (synchronous): for a transport of the caller's own. */
int catchhip_shard_buffer_copy(catchhip_shard *shard, int32_t which, void *host,
                               int32_t to_host);
int catchhip_shard_allreduce_local(int32_t n, catchhip_shard *const *shards,
                                   int32_t which);
/* The whole round loop of a sharded instance in one call (round 6; catch_amd/parallel.py drove it from the
 * interpreter, one host synchronisation per round, until then): count -> all-reduce SUM -> claim -> all-reduce MAX ->
 * [partial coverage: verdict -> all-reduce MAX] -> apply, queued stream-ordered rounds_per_sync rounds at a time; the
 * exchange buffers keep the capacity of the last read-back, the done flag and the number of sets still alive are read
 * back once per batch (the step functions above are batches of one round).  shards: the n <= 64 shards this process
 * holds, fresh (round 0); transport 0: RCCL over the
 * context's communicator (one shard per process, one process per GPU: the production path, replaces the worker pool
 * of catch/filter/set_cover_filter.py:848-900 for a group that is sharded), 1: the shards of this process exchange
 * among themselves (one context; tests, and one-GPU runs of several ranges).  *done: 1 finished, -1 rank list
 * exhausted; catchhip_shard_picks then returns the picks. */
int catchhip_shard_solve(int32_t n, catchhip_shard *const *shards, int32_t transport, int32_t rounds_per_sync,
                         int32_t *done);

/* ---- K3: near-duplicate filter (Hamming LSH) --------------------------- */
/* Replaces NearDuplicateFilter._filter for NearDuplicateFilterWithHamming
 * Distance (catch/filter/near_duplicate_filter.py:47-142) with
 * lsh.NearNeighborLookup (catch/utils/lsh.py:239-320): n UNIQUE probes of
 * equal length L given in priority order (multiplicity descending, stable);
 * positions[ntables*k] the sampled positions per table; keep[n] (host,
 * uint8) receives 1 for probes that the sequential greedy pass includes. */
int catchhip_ndf_hamming(catchhip_ctx *ctx, const uint8_t *bytes, int64_t n,
                         int32_t L, const int32_t *positions, int32_t ntables,
                         int32_t k, int32_t dist_thres, uint8_t *keep);

/* Replaces NearDuplicateFilter._filter for NearDuplicateFilterWithMinHash
 * (catch/filter/near_duplicate_filter.py:148-190) with lsh.MinHashFamily(
 * kmer_size, N=1, use_fast_str_hash=True) and lsh.NearNeighborLookup
 * (catch/utils/lsh.py:48-215, :239-320).  The family's inner hash is the
 * interpreter's hash(str); this library computes it as CPython <= 3.10 does
 * under PYTHONHASHSEED=0 (SipHash-2-4, zero key) -- the only setting that
 * makes the reference's filter reproducible, and the one the golden vectors
 * were recorded with.  n UNIQUE probes in priority order (bytes / probe_off[n+1];
 * lengths may differ, each >= kmer_size <= 16, at most 256 k-mers per probe);
 * ab[ntables*k*2] = (a, b) of every hash function in the order the reference
 * draws them; a table key is the tuple of k minima of (a*|hash(kmer)|+b) mod
 * (2^31-1); two probes are near-duplicates when they share a key in some table
 * and the Jaccard distance of their k-mer sets (float64) is <= dist_thres. */
int catchhip_ndf_minhash(catchhip_ctx *ctx, const uint8_t *bytes,
                         const int64_t *probe_off, int64_t n, int32_t kmer_size,
                         const int64_t *ab, int32_t ntables, int32_t k,
                         double dist_thres, uint8_t *keep);

/* The same filter for `ngroups` independent groups of probes in one pass (the
 * clusters of --cluster-and-design-separately; BaseFilter.filter runs _filter
 * once per group, catch/filter/base_filter.py:111-175): group g = probes
 * [group_off[g], group_off[g+1]) in priority order, with its own hash functions
 * ab[g][ntables][k][2]; no probe is compared with a probe of another group. */
int catchhip_ndf_minhash_many(catchhip_ctx *ctx, const uint8_t *bytes,
                              const int64_t *probe_off, int64_t n,
                              const int64_t *group_off, int64_t ngroups,
                              int32_t kmer_size, const int64_t *ab,
                              int32_t ntables, int32_t k, double dist_thres,
                              uint8_t *keep);

/* ---- clustering pre-step (next row: catch/utils/cluster.py) --------------
 * MinHash signatures of sequences, replacing lsh.MinHashFamily(kmer_size, N)
 * .make_h() / h(s) (catch/utils/lsh.py:75-153) with the deterministic md5 inner
 * hash (:106-111) as cluster.make_signatures_with_minhash calls it
 * (catch/utils/cluster.py:28-44): per sequence the N smallest values, with
 * multiplicity, ascending, of (a * md5(kmer) + b) mod (2^31 - 1) over all
 * k-mers (md5 digest read as a big-endian 128-bit integer); a sequence with
 * fewer than N k-mers repeats them in whole rounds.  bytes = the sequences'
 * characters back to back (ASCII, as given -- no case folding), offsets[nseq+1]
 * their starts; 1 <= kmer_size <= 55 <= every sequence length; N <= 1024;
 * (a, b) as the reference draws them (1 <= a <= 2^31-1, 0 <= b <= 2^31-1). */
typedef struct catchhip_sigs catchhip_sigs;
int catchhip_sigs_create(catchhip_ctx *ctx, const uint8_t *bytes,
                         const uint64_t *offsets, uint32_t nseq,
                         int32_t kmer_size, uint32_t N, uint32_t a, uint32_t b,
                         catchhip_sigs **out);
/* The same with one pointer per sequence (the strings' own storage, e.g. CPython's ASCII str
 * buffers): gathered by host threads into pinned memory -- no multi-gigabyte join on the caller's side. */
int catchhip_sigs_create_ptrs(catchhip_ctx *ctx, const uint8_t *const *seq_ptr, const int64_t *seq_len,
                              uint32_t nseq, int32_t k, uint32_t N, uint32_t a, uint32_t b,
                              catchhip_sigs **out);
void catchhip_sigs_destroy(catchhip_sigs *sigs);
/* out[nseq * N]: signature of sequence s at out[s*N .. s*N+N) */
int catchhip_sigs_fetch(catchhip_ctx *ctx, const catchhip_sigs *sigs,
                        uint32_t *out);
/* MinHashFamily.estimate_jaccard_dist (catch/utils/lsh.py:170-215) of signature
 * j against every signature: common[k] = values the merge walk finds in both
 * (the walk always makes exactly N union steps, so the reference's distance is
 * 1.0 - common[k] / N in float64, which the caller forms). */
int catchhip_sigs_common_row(catchhip_ctx *ctx, const catchhip_sigs *sigs,
                             uint32_t j, uint16_t *common);
/* The same row reduced to the neighbours the connected-components search
 * (catch/utils/cluster.py:235-355) looks at: out[i] = (k << 16 | common[k]) for
 * every sequence k with common[k] >= min_common (its distance to j is within the
 * threshold), in no particular order; *count = how many (an error when it
 * exceeds cap).  Signatures of at most 176 values. */
int catchhip_sigs_neighbors(catchhip_ctx *ctx, const catchhip_sigs *sigs,
                            uint32_t j, uint32_t min_common,
                            unsigned long long *out, int64_t cap, int64_t *count);
/* The lists of up to 32 vertices in one launch (the search asks for the vertex it
 * explores together with those it has just stacked): out[i] = (q << 48 | k << 16 |
 * common[k]) for query q = js[q].  Signatures of at most 112 values.  *count beyond cap is
 * an error (CATCHHIP_EINVAL; nothing is written to out then). */
int catchhip_sigs_neighbors_many(catchhip_ctx *ctx, const catchhip_sigs *sigs,
                                 const uint32_t *js, int64_t nq, uint32_t min_common,
                                 unsigned long long *out, int64_t cap, int64_t *count);
/* The neighbour lists of ALL vertices at once (the graph the connected-components search of
 * catch/utils/cluster.py:235-355 walks): every ordered pair (j, k), j != k, with common(j, k) >= min_common.
 * Built and kept on the device; *nedges = how many.  max_edges > 0: when the graph has more, nothing is kept
 * (the caller falls back to catchhip_sigs_neighbors_many).  Signatures of at most 112 values. */
int catchhip_sigs_graph(catchhip_ctx *ctx, catchhip_sigs *sigs, uint32_t min_common,
                        int64_t max_edges, int64_t *nedges);
/* ... copied out in CSR form: the neighbours of j are idx[ptr[j] .. ptr[j + 1]) ascending, common[] beside them. */
int catchhip_sigs_graph_fetch(catchhip_ctx *ctx, const catchhip_sigs *sigs, int64_t *ptr,
                              uint32_t *idx, uint32_t *common);
/* The connected-components search of catch/utils/cluster.py:235-355 over such a graph, host side (no kernel):
 * runs the explored vertices whose neighbour order is known without building a Python set (catch_amd/utils/
 * cluster.py says when) and hands the others back.  ptr / idx / common are borrowed until catchhip_dfs_destroy;
 * a neighbour with common >= near_common is absorbed without being explored (the early-stop rule, :313-330).
 * catchhip_dfs_run(m = len(remaining)): *status 0 = finished; 1 = a component ended (catchhip_dfs_seen lists it;
 * remove it from `remaining`, run again); 2 = catchhip_dfs_set_copy_rank is needed (rank of every vertex in the
 * iteration order of remaining.copy()), run again; 3 = *vertex needs a real `remaining - queued`
 * (catchhip_dfs_new_queued lists what was queued since the last call; catchhip_dfs_push files the vertex's
 * neighbours in that set's order), run again.  catchhip_dfs_counts: explored vertices by case. */
typedef struct catchhip_dfs catchhip_dfs;
int catchhip_dfs_create(uint32_t n, const int64_t *ptr, const uint32_t *idx, const uint32_t *common,
                        uint32_t near_common, catchhip_dfs **out);
void catchhip_dfs_destroy(catchhip_dfs *dfs);
int catchhip_dfs_run(catchhip_dfs *dfs, int64_t m, int32_t *status, int64_t *vertex);
int catchhip_dfs_seen(catchhip_dfs *dfs, const uint32_t **p, int64_t *count);
int catchhip_dfs_new_queued(catchhip_dfs *dfs, const uint32_t **p, int64_t *count);
int catchhip_dfs_set_copy_rank(catchhip_dfs *dfs, const int64_t *rank);
/* the same from the members of remaining.copy() in its iteration order (a member's rank is its position) */
int catchhip_dfs_set_copy_members(catchhip_dfs *dfs, const int64_t *members, int64_t count);
int catchhip_dfs_push(catchhip_dfs *dfs, const int64_t *ks, const uint8_t *near, int64_t count);
int catchhip_dfs_counts(const catchhip_dfs *dfs, int64_t *out3);
/* The whole search in one call (round 6; nothing is handed back to the interpreter): `indices_to_consider`
 * (catch/utils/cluster.py:284, :343) is kept as CPython lays it out -- set(range(n)), `-=` with its dummies and
 * rebuilds, copy(), and the difference built insert by insert -- so the order of `list(a - b)` (:303-304) is the
 * interpreter's.  On a fresh handle.  comp[n]: vertices component after component in discovery order;
 * comp_ptr[n + 1]; stats[8] (may be null): explored vertices by the case of their difference (ascending, a copy of
 * the set, built insert by insert), how many of them had fewer than two new neighbours (no order to establish),
 * copies simulated, differences simulated, keys those inserted, orders read off the keys' home slots (the members
 * span fewer keys than the table has slots). */
int catchhip_dfs_run_all(catchhip_dfs *dfs, uint32_t *comp, int64_t *comp_ptr, int64_t *ncomp, int64_t *stats);
/* The emulated set by itself, for checking it against the interpreter (catch_amd/utils/cluster.py does so once per
 * process): create = set(range(n)); isub: s -= set(keys); list(which = 0: list(s), 1: list(s.copy()),
 * 2: list(s - set(keys))) -> *p (valid until the next call on the handle), *count. */
typedef struct catchhip_pyintset catchhip_pyintset;
int catchhip_pyintset_create(uint32_t n, catchhip_pyintset **out);
void catchhip_pyintset_destroy(catchhip_pyintset *s);
int catchhip_pyintset_isub(catchhip_pyintset *s, const uint32_t *keys, int64_t count);
int catchhip_pyintset_list(catchhip_pyintset *s, int32_t which, const uint32_t *keys, int64_t count,
                           const uint32_t **p, int64_t *n);
/* cluster.create_condensed_dist_matrix (catch/utils/cluster.py:102-194) for the
 * signature distance: out[n(n-1)/2] float32 in SciPy's condensed order, entry
 * (i, j) = lut[common(i, j)] with lut[N+1] supplied by the caller (the float32
 * roundings of 1.0 - c / N, which is what the reference's c_float array holds). */
int catchhip_sigs_condensed(catchhip_ctx *ctx, const catchhip_sigs *sigs,
                            const float *lut, float *out);
/* cluster.cluster_hierarchically_from_dist_matrix (catch/utils/cluster.py:197-232) on the device: SciPy's
 * linkage(method="average") -- the nearest-neighbour chain in float64 with its tie rules, one persistent workgroup --
 * and fcluster(criterion="distance") at `threshold`.  The distances are those of catchhip_sigs_condensed
 * ((double)lut[common(i, j)]; the float32 matrix is never written), or a caller's float32 condensed matrix of n points,
 * n (n - 1) / 2 entries, all finite (CATCHHIP_EINVAL otherwise, as SciPy raises ValueError).  labels[n]: SciPy's
 * 1-based flat cluster numbers.  merges[(n - 1) * 4] (may be null): the linkage matrix as SciPy returns it -- sorted
 * by height (stable), relabelled so that merge k creates node n + k.  Needs 8 n^2 bytes of device memory. */
int catchhip_sigs_linkage_average(catchhip_ctx *ctx, const catchhip_sigs *sigs, const float *lut,
                                  double threshold, int32_t *labels, double *merges);
int catchhip_linkage_average(catchhip_ctx *ctx, int64_t n, const float *condensed, double threshold,
                             int32_t *labels, double *merges);
/* The host part of the two by itself (no device): merges[(n - 1) * 4] = (x, y, height, size) per merge in the order
 * the chain made them, x and y the points that stand for the two clusters -> labels[n] and sorted[(n - 1) * 4]
 * (may be null) as above. */
int catchhip_linkage_labels(int64_t n, const double *merges, double threshold, int32_t *labels, double *sorted);
/* *fits = 1 when the float64 square matrix of n points takes at most half of the device memory that is free now. */
int catchhip_linkage_fits(catchhip_ctx *ctx, int64_t n, int32_t *fits);

/* ---- scan with first-discovery keys (next row: catch/filter/adapter_filter.py)
 * catchhip_cover_scan, plus for every row the key that orders probes the way
 * the reference's result dict does: find_probe_covers_in_sequence walks a
 * sequence left to right, looks every k-mer up in the k-mer -> {(probe, pos)}
 * map and inserts a probe into its result when the first of its seeds is
 * accepted (catch/probe.py:1062-1108, :1253-1271); AdapterFilter's interval
 * scheduling breaks ties between equal range ends by that insertion order
 * (catch/filter/adapter_filter.py:191-240, catch/utils/interval.py:319-358).
 * Per (set, universe) group: first_key = (position of that first accepted k-mer
 * relative to the universe's start) << 32 | anchor_order[entry], where
 * anchor_order[nanchors] (may be null = 0) is the caller's rank of each anchor
 * entry inside its k-mer's entry list (the reference iterates a Python set
 * there; the host mirrors it).  The probes must have been created with their
 * anchors sorted by (probe, position) without duplicates; give every sequence
 * its own universe to get per-sequence keys.  Not available with
 * CATCHHIP_SCAN_FAST. */
int catchhip_cover_scan_first_seen(catchhip_ctx *ctx, const catchhip_probes *probes,
                                   const catchhip_targets *targets,
                                   int32_t mismatches, int32_t lcf_thres,
                                   int32_t island_of_exact_match,
                                   int32_t cover_extension, int32_t mode,
                                   const uint32_t *anchor_order,
                                   catchhip_rows **out, int64_t *nrows);
/* first_key[nrows], aligned with catchhip_rows_fetch */
int catchhip_rows_fetch_first_seen(catchhip_ctx *ctx, const catchhip_rows *rows,
                                   uint64_t *first_key);

/* ---- independent instances in one scan ------------------------------------
 * The groups of a design are independent set cover instances
 * (catch/filter/set_cover_filter.py:816-846: _make_sets per group, one solve
 * per group).  Many small groups (the clusters of
 * --cluster-and-design-separately) can share one probes / targets pair: give
 * every probe and every genome the number of its group; the scans then report
 * a probe only inside genomes of its own group.  The rows of the groups are
 * disjoint in sets and universes, so one greedy solve over all of them makes,
 * restricted to a group, exactly that group's own sequence of picks (a set's
 * gain depends only on its own group's universes; ties go to the lowest id).
 * Pass null to remove the groups. */
int catchhip_probes_set_groups(catchhip_ctx *ctx, catchhip_probes *probes,
                               const int32_t *group_of_probe);
int catchhip_targets_set_groups(catchhip_ctx *ctx, catchhip_targets *targets,
                                const int32_t *group_of_genome);

/* ---- candidate probes on the device (front end, next row #1) ---------------
 * candidate_probes.make_candidate_probes_from_sequences over all sequences of a
 * targets object, genome by genome (catch/filter/candidate_probes.py:21-182 as
 * ProbeDesigner calls it, catch/filter/probe_designer.py:250-262: windows of
 * probe_length every probe_stride bases, the window flush with the sequence end
 * when the length is not a multiple of the stride, no window holding two or
 * more consecutive 'N', and the windows flanking every run of >= 2 'N'),
 * followed by DuplicateFilter (catch/filter/duplicate_filter.py:16-26: first
 * occurrences, order kept).  The unique candidates stay on the device as
 * positions in the targets; their index in first-occurrence order is the set id
 * the set cover works with.  seq_length_to_skip < 0 = none; a sequence shorter
 * than probe_length that is not skipped is an error, as in the reference
 * (--small-seq-min is handled by the host's string path).  `targets` must
 * outlive the candidates object. */
typedef struct catchhip_candidates catchhip_candidates;
int catchhip_candidates_create(catchhip_ctx *ctx, const catchhip_targets *targets,
                               int32_t probe_length, int32_t probe_stride,
                               int64_t seq_length_to_skip,
                               catchhip_candidates **out, int64_t *ncandidates,
                               int64_t *nunique);
void catchhip_candidates_destroy(catchhip_candidates *cands);
/* Iteration order of a CPython set.  The reference's near-duplicate filters
 * return `list(to_include)` -- a set of Probe objects hashed by hash(seq_str)
 * (catch/filter/near_duplicate_filter.py:76-103, catch/probe.py:324-329) -- and
 * SetCoverFilter numbers its candidates in the order it receives them, so which of
 * two equally good probes is picked follows from that order.  order[i] = index of
 * the i-th key a set iterates after the n distinct keys with these hashes were added
 * in index order (Objects/setobject.c of CPython 3.7-3.12).  ..._strs hashes the
 * strings as CPython <= 3.10 does under PYTHONHASHSEED=0 (SipHash-2-4, zero key) --
 * the one setting under which the reference's own order is reproducible; the
 * catchhip_candidates_ndf_* calls leave their candidates in this order.
 * Host-only integer work (no device involved). */
int catchhip_pyset_order(const int64_t *hashes, int64_t n, int64_t *order);
int catchhip_pyset_order_strs(const uint8_t *bytes, const int64_t *off, int64_t n,
                              int64_t *order);
/* The same order computed on the device (what the catchhip_candidates_ndf_* calls use for
 * more than a few thousand kept probes): all insertions of one table generation at once,
 * a slot claimed with atomicMin on (insertion rank, index) words and the displaced key
 * walking on -- the fixed point is the sequential table.  hashes / order: host arrays. */
int catchhip_pyset_order_device(catchhip_ctx *ctx, const int64_t *hashes, int64_t n, int64_t *order);
int catchhip_candidates_rebind(catchhip_candidates *cands, catchhip_ctx *to);   /* see catchhip_targets_rebind */
/* global_start[i] = position (in the targets' concatenated coordinate) of the
 * first occurrence of unique candidate ids[i] (ids == NULL: candidates 0..n-1) */
int catchhip_candidates_fetch(catchhip_ctx *ctx, const catchhip_candidates *cands,
                              const int64_t *ids, int64_t n, int64_t *global_start);
/* NearDuplicateFilter._filter on the candidates (catch/filter/
 * near_duplicate_filter.py:47-103; arguments as catchhip_ndf_hamming /
 * catchhip_ndf_minhash): the unique candidates are taken in the filters'
 * priority order -- multiplicity among ALL candidates descending, ties in
 * first-occurrence order (:60-66) -- and the object's list becomes the kept
 * ones in that order, which is the order the set cover filter then numbers
 * them in.  At most one such call per candidates object. */
int catchhip_candidates_ndf_hamming(catchhip_ctx *ctx, catchhip_candidates *cands,
                                    const int32_t *positions, int32_t ntables,
                                    int32_t k, int32_t dist_thres, int64_t *nkept);
int catchhip_candidates_ndf_minhash(catchhip_ctx *ctx, catchhip_candidates *cands,
                                    int32_t kmer_size, const int64_t *ab,
                                    int32_t ntables, int32_t k, double dist_thres,
                                    int64_t *nkept);
/* Grouped targets (catchhip_targets_set_groups before catchhip_candidates_create):
 * duplicates are only removed inside a group, the candidates of a group stay
 * together (groups in order), the priority order is per group, and
 * catchhip_probes_from_candidates passes the groups on to the probes.  The
 * near-duplicate filters then take one set of sampled positions / hash
 * functions per group (ab[ngroups][ntables][k][2] as catchhip_ndf_minhash_many);
 * catchhip_candidates_groups returns the group of every unique candidate. */
int catchhip_candidates_ndf_hamming_many(catchhip_ctx *ctx, catchhip_candidates *cands,
                                         const int32_t *positions /* [ngroups][ntables][k] */,
                                         int64_t ngroups, int32_t ntables, int32_t k,
                                         int32_t dist_thres, int64_t *nkept);
int catchhip_candidates_ndf_minhash_many(catchhip_ctx *ctx, catchhip_candidates *cands,
                                         int32_t kmer_size, const int64_t *ab,
                                         int64_t ngroups, int32_t ntables, int32_t k,
                                         double dist_thres, int64_t *nkept);
int catchhip_candidates_groups(catchhip_ctx *ctx, const catchhip_candidates *cands,
                               int32_t *group_of_candidate);
/* PolyAFilter._filter on the candidates (catch/filter/polya_filter.py:43-71, which
 * costs a k_lcf call of O(L^2) per candidate): unique candidates with a stretch of
 * >= length 'A' (or 'T') under `mismatches` mismatches are dropped -- but only
 * those that hold an exact run of >= min_exact 'A' or 'T', the reference's gate
 * (min_exact_length_to_consider, 6 by default; 0 = no gate).  Every character but
 * the stretch's own is a mismatch, N included; length > probe_length drops nothing.
 * The rule is a function of the candidate alone, so the list left -- order,
 * multiplicities and groups kept, ncandidates untouched -- is what the reference's
 * [PolyAFilter, DuplicateFilter] leaves.  Before any catchhip_candidates_ndf_* call
 * (EINVAL after one); grouped and ungrouped candidates alike; *nkept = candidates
 * left (0 is valid). */
int catchhip_candidates_drop_polya(catchhip_ctx *ctx, catchhip_candidates *cands,
                                   int32_t length, int32_t mismatches,
                                   int32_t min_exact, int64_t *nkept);
/* NOT IN THE REFERENCE (catch_amd/filter/composition_filter.py states the rules and
 * is their oracle): unique candidates that fail a composition rule are dropped, as
 * catchhip_candidates_drop_polya drops its own -- order, multiplicities and groups
 * kept, before any near-duplicate filter (EINVAL after one), 0 candidates valid.
 * Only the bytes 'A', 'C', 'G', 'T' are bases; L = probe_length.
 *   GC: kept iff gc_lo <= number of 'G' or 'C' <= gc_hi (gc_lo = -1: no lower bound,
 *       gc_hi = -1: no upper bound; gc_lo <= 0 with gc_hi >= L is "off" as well).
 *   homopolymer: kept iff the longest run of one base is <= max_run (>= 1; -1: off).
 *   low complexity: with We = min(dust_window, L), dropped iff for some window start
 *       i in 0 .. L - We the triplets j in i .. i + We - 3 whose three bytes are all
 *       bases -- T of them, c_t with code t -- have T >= 2 and
 *       10 * sum_t c_t (c_t - 1) / 2 > dust_x10 * (T - 1)  (dust_x10 >= 0; -1: off;
 *       3 <= dust_window <= 256, read only when the rule is on).
 * dropped (4 words, may be NULL) receives the candidates each rule dropped, counted
 * WITH multiplicity: [0] GC, [1] homopolymer, [2] low complexity, [3] any rule (a
 * candidate that fails two rules counts for both and once in [3]). */
int catchhip_candidates_drop_composition(catchhip_ctx *ctx, catchhip_candidates *cands,
                                         int32_t gc_lo, int32_t gc_hi, int32_t max_run,
                                         int32_t dust_x10, int32_t dust_window,
                                         int64_t dropped[4], int64_t *nkept);
/* NOT IN THE REFERENCE (catch_amd/filter/structure_filter.py states the rules and is
 * their oracle): unique candidates that fail a secondary-structure rule are dropped,
 * as catchhip_candidates_drop_composition drops its own -- order, multiplicities and
 * groups kept, before any near-duplicate filter (EINVAL after one), 0 candidates
 * valid.  Only the bytes 'A', 'C', 'G', 'T' are bases; pairs(x, y) iff both are bases
 * and complementary (A-T, C-G); L = probe_length.
 *   hairpin: dropped iff there are i < j with pairs(i + t, j - t) for t = 0 .. max_stem
 *       and (j - max_stem) - (i + max_stem) - 1 >= min_loop  (max_stem >= 1; -1: off;
 *       min_loop >= 0, read only when the rule is on).
 *   self-dimer: dropped iff there are a, b with 0 <= a, a + max_dimer <= L - 1,
 *       b - max_dimer >= 0, b <= L - 1 and pairs(a + t, b - t) for t = 0 .. max_dimer
 *       (max_dimer >= 1; -1: off).
 * dropped (3 words, may be NULL) receives the candidates each rule dropped, counted
 * WITH multiplicity: [0] hairpin, [1] self-dimer, [2] any rule (a candidate that fails
 * both counts for both and once in [2]).  The flag kernel is phase 9 of
 * catchhip_ctx_last_kernel_ms. */
int catchhip_candidates_drop_structure(catchhip_ctx *ctx, catchhip_candidates *cands,
                                       int32_t max_stem, int32_t min_loop, int32_t max_dimer,
                                       int64_t dropped[3], int64_t *nkept);
/* NOT IN THE REFERENCE (catch_amd/filter/tm_filter.py states the rule and is its
 * oracle): the nearest-neighbour melting temperature of every unique candidate, as a
 * filter and as a histogram.  With H and E the sums of the unified parameters of
 * SantaLucia 1998 over the candidate's dinucleotides and its two terminal characters
 * (h in 100 cal/mol, e in 0.1 cal/(K mol); only 'A', 'C', 'G', 'T' are bases, a
 * dinucleotide with another byte adds nothing),
 *     E' = 100 E + q,  T = H < 0 ? floor(10^7 (-H) / (-E')) : 0,  tm_c = T - offset_c
 * in 64-bit integers: q = Q(probe_length), the salt and concentration term the caller
 * computes once, q <= -8200 (EINVAL otherwise); offset_c = 27315 + f, f the formamide
 * correction; tm_c is in hundredths of a degree Celsius.
 *   filter_on != 0: candidates with tm_c < lo_c or tm_c > hi_c are dropped (EINVAL if
 *       lo_c > hi_c), as catchhip_candidates_drop_composition drops its own -- order,
 *       multiplicities and groups kept, before any near-duplicate filter (EINVAL after
 *       one), 0 candidates valid; nothing dropped: the list stands as it is.
 *   filter_on == 0: the list is untouched; lo_c and hi_c are not read.
 * dropped (3 words, may be NULL) receives the candidates dropped, counted WITH
 * multiplicity: [0] below lo_c, [1] above hi_c, [2] both together.  hist (128 words,
 * may be NULL) receives the candidates the call saw, before it dropped any, WITH
 * multiplicity, per whole degree: bin min(max(floor(tm_c / 100), 0), 127).
 * probe_length < 2: nothing is dropped and nothing counted.  The flag kernel is phase 9
 * of catchhip_ctx_last_kernel_ms. */
int catchhip_candidates_drop_tm(catchhip_ctx *ctx, catchhip_candidates *cands, int64_t q,
                                int32_t offset_c, int32_t filter_on, int32_t lo_c,
                                int32_t hi_c, int64_t dropped[3], uint64_t hist[128],
                                int64_t *nkept);
/* NOT IN THE REFERENCE (catch_amd/filter/background_filter.py states the rule and is
 * its oracle): an index of the k-mers of a background -- the sequences probes must not
 * match -- for catchhip_candidates_drop_background.
 *   bytes, off[nseq + 1]: the records side by side, record i = bytes[off[i] .. off[i+1]),
 *       off[0] = 0; only 'A', 'C', 'G', 'T' are bases, a k-mer is valid iff its k bytes
 *       are bases and lie in ONE record; 8 <= k <= 32 (EINVAL otherwise).
 *   code of a k-mer: 2 bits per character, (c >> 1) & 3 ('A' 0, 'C' 1, 'T' 2, 'G' 3), the
 *       first character in the most significant of the 2k bits of a uint64_t; the
 *       complement of a code is code ^ 2; canonical(w) = the smaller of code(w) and
 *       code(reverse complement of w), unsigned.
 * The index holds the sorted distinct canonical codes of the valid k-mers and a prefix
 * directory over them, in device memory of its own (not a context's block cache): every
 * context of ctx's device may use it, and it outlives ctx.  *n_valid = valid k-mer
 * positions, *n_unique = distinct canonical codes (either may be NULL).  nseq = 0, records
 * shorter than k and records without a valid k-mer are fine: an empty index.  A background
 * of 2^32 - 4096 bytes or more is refused (EINVAL): the build sorts and scans with 32-bit
 * counts, so 2^32 valid positions and more cannot be indexed in one piece.  The build
 * takes about 24 bytes of scratch from ctx's pool per valid position, the index keeps
 * 8 bytes per distinct code plus the directory (4 bytes per entry, about one entry per
 * code).  The call synchronises before it returns; its kernels are phase 9 of
 * catchhip_ctx_last_kernel_ms, from behind the upload on. */
typedef struct catchhip_kmer_index catchhip_kmer_index;
int catchhip_kmer_index_create(catchhip_ctx *ctx, const uint8_t *bytes, const int64_t *off,
                               int64_t nseq, int32_t k, catchhip_kmer_index **index,
                               int64_t *n_valid, int64_t *n_unique);
/* out[0 .. n_unique): the sorted distinct canonical codes; ctx: any context of the
 * index's device */
int catchhip_kmer_index_fetch(catchhip_ctx *ctx, const catchhip_kmer_index *index,
                              uint64_t *out);
/* frees the index's device memory (waits for the device's work); NULL is fine */
void catchhip_kmer_index_destroy(catchhip_kmer_index *index);
/* NOT IN THE REFERENCE (catch_amd/filter/background_filter.py states the rule): the index
 * of catchhip_kmer_index_create for matching within `mismatches` = M substitutions, M in
 * 0 .. 2 and k >= 8 (M + 1) (EINVAL otherwise).  M = 0 builds exactly what
 * catchhip_kmer_index_create builds.  M > 0: block b = 0 .. M of a k-mer is its characters
 * [s_b, s_(b+1)), s_b = floor(b k / (M + 1)); two k-mers at most M mismatches apart agree
 * in one block.  The index holds M + 1 VIEWS of the distinct canonical codes: view b is
 * every code rotated left by 2 s_b bits inside its 2k bits (block b in the most
 * significant bits; view 0 is the codes as they are), sorted, with a directory of its own
 * of P_b = clamp(ceil(log2 n_unique), 8, min(2 (s_(b+1) - s_b), 30)) bits -- never finer
 * than the block, so one bucket holds every code that agrees with a query in block b.
 * 8 (M + 1) bytes per distinct code plus the directories.  The mismatch budget travels in
 * the index: catchhip_candidates_drop_background and catchhip_candidates_measure count a
 * k-mer w as a hit iff some code c of the index lies within M mismatches of code(w) or of
 * code(reverse complement of w). */
int catchhip_kmer_index_create_tolerant(catchhip_ctx *ctx, const uint8_t *bytes,
                                        const int64_t *off, int64_t nseq, int32_t k,
                                        int32_t mismatches, catchhip_kmer_index **index,
                                        int64_t *n_valid, int64_t *n_unique);
/* NOT IN THE REFERENCE: out[0 .. n_unique): the sorted rotated codes of one view, 0 <= view
 * <= the index's mismatches (EINVAL otherwise); view 0 is what catchhip_kmer_index_fetch
 * returns */
int catchhip_kmer_index_fetch_view(catchhip_ctx *ctx, const catchhip_kmer_index *index,
                                   int32_t view, uint64_t *out);
/* NOT IN THE REFERENCE (catch_amd/filter/background_filter.py): the background k-mer
 * screen on the unique candidates, as a filter and as a histogram.  w HITS iff w or its
 * reverse complement is a valid k-mer of the background, i.e. iff canonical(w) is in the
 * index; hits(s) = the positions j in 0 .. probe_length - k whose k-mer s[j .. j + k) is
 * valid (k bases, bytes as they are) and hits.
 *   filter_on != 0: candidates with hits > max_hits are dropped (max_hits >= 0, EINVAL
 *       otherwise), as catchhip_candidates_drop_tm drops its own -- order, multiplicities
 *       and groups kept, before any near-duplicate filter (EINVAL after one), 0 candidates
 *       valid; nothing dropped: the list stands as it is.
 *   filter_on == 0: the list is untouched; max_hits is not read.
 * dropped (1 word, may be NULL) receives the candidates dropped, counted WITH
 * multiplicity.  hist (256 words, may be NULL) receives the candidates the call saw,
 * before it dropped any, WITH multiplicity, per hit count: bin min(hits, 255).  An empty
 * index drops nothing and counts every candidate in bin 0.  probe_length < k: nothing is
 * dropped and nothing counted; neither then nor with 0 candidates nor with filter_on == 0
 * and hist == NULL is anything launched.  ctx must be the candidates' context and the
 * index must live on its device (EINVAL otherwise); the index may have been built on
 * another context of that device.  The flag kernel is phase 9 of
 * catchhip_ctx_last_kernel_ms. */
int catchhip_candidates_drop_background(catchhip_ctx *ctx, catchhip_candidates *cands,
                                        const catchhip_kmer_index *index, int32_t filter_on,
                                        int64_t max_hits, int64_t dropped[1],
                                        uint64_t hist[256], int64_t *nkept);
/* NOT IN THE REFERENCE (catch_amd/filter/quality.py states the five quantities and is
 * their oracle): the value behind every candidate rule, for every unique candidate, as
 * per-candidate arrays and as histograms.  The list is only read: order, multiplicities
 * and groups stay exactly as they were.  Before any near-duplicate filter (EINVAL after
 * one), 0 candidates valid.  Only the bytes 'A', 'C', 'G', 'T' are bases.
 *   what: a mask of the families to compute; 0 is valid and computes nothing.
 *     CATCHHIP_MEASURE_COMPOSITION  gc (number of 'G' or 'C'), homopolymer (longest run of
 *         one base) and dust (the smallest dust_x10 at which
 *         catchhip_candidates_drop_composition keeps the candidate: the maximum over its
 *         windows with T >= 2 of ceil(10 S / (T - 1)), 0 without one; 3 <= dust_window <= 256)
 *     CATCHHIP_MEASURE_STRUCTURE    stem (the base pairs of the longest hairpin stem around
 *         a loop of at least min_loop >= 0 characters: catchhip_candidates_drop_structure
 *         drops the candidate iff stem > max_stem) and dimer (the longest run of
 *         consecutive base pairs of two copies: dropped iff dimer > max_dimer); 0 if none
 *     CATCHHIP_MEASURE_TM           tm_c of catchhip_candidates_drop_tm with the same q (<= -8200)
 *         and offset_c, clamped to +-(2^31 - 1); CATCHHIP_MEASURE_NO_TM for probe_length < 2
 *     CATCHHIP_MEASURE_HITS         hits of catchhip_candidates_drop_background against
 *         index (of ctx's device, EINVAL otherwise; not read without this bit); 0 for
 *         probe_length < k
 *   want_values != 0: gc, homopolymer, dust, stem, dimer, tm_c and hits (host arrays of one
 *       entry per unique candidate) receive the values of the families asked for; the
 *       arrays of the other families are not touched and may be NULL.  want_values == 0:
 *       none of the seven is read.
 *   hist (5 * 1280 words, may be NULL) receives five histograms over the candidates, WITH
 *       multiplicity: words [1280 q, 1280 q + 1280) for q = gc, homopolymer, dust, stem,
 *       dimer in this order, bin min(value, 1279); the histograms of a family not asked
 *       for are 0.  Tm and hits have histograms of their own in their filter calls.
 * probe_length > 65,535 is refused (EINVAL): the five values are 16-bit.  The kernels are
 * phase 9 of catchhip_ctx_last_kernel_ms. */
#define CATCHHIP_MEASURE_COMPOSITION 1u
#define CATCHHIP_MEASURE_STRUCTURE 2u
#define CATCHHIP_MEASURE_TM 4u
#define CATCHHIP_MEASURE_HITS 8u
#define CATCHHIP_MEASURE_NO_TM (-2147483647 - 1)
int catchhip_candidates_measure(catchhip_ctx *ctx, const catchhip_candidates *cands,
                                uint32_t what, int32_t min_loop, int32_t dust_window,
                                int64_t q, int32_t offset_c, const catchhip_kmer_index *index,
                                int32_t want_values, uint16_t *gc, uint16_t *homopolymer,
                                uint16_t *dust, uint16_t *stem, uint16_t *dimer,
                                int32_t *tm_c, uint32_t *hits, uint64_t *hist);
/* multiplicity[i] = how many candidates equal unique candidate i (the priority of
 * near_duplicate_filter.py:60-66); EINVAL once a catchhip_candidates_ndf_* call ran */
int catchhip_candidates_multiplicities(catchhip_ctx *ctx, const catchhip_candidates *cands,
                                       uint32_t *multiplicity);
/* A probes object of the unique candidates (set id = candidate index), as
 * catchhip_probes_create would build from their strings.  Anchors: sorted by
 * (probe, position) without duplicates, or ent_probe = ent_pos = NULL for the
 * pigeonhole table {0, k, 2k, ..} of every probe (k must divide probe_length). */
int catchhip_probes_from_candidates(catchhip_ctx *ctx, const catchhip_candidates *cands,
                                    const int32_t *ent_probe, const int32_t *ent_pos,
                                    int64_t nent, int32_t k, catchhip_probes **out);
/* The same with RANDOM anchors given as their draws (catch/probe.py:356-405:
 * construct_kmer_probe_map_to_find_probe_covers draws num_kmers_per_probe = 20
 * positions per probe with np.random, repeats allowed; the map keeps a probe
 * once per distinct k-mer position): draws[probe][draws_per_probe], one byte
 * each (probe_length - k + 1 <= 256), in the order np.random.randint made them.
 * The table is every probe's sorted distinct positions, built on the device. */
int catchhip_probes_from_candidates_draws(catchhip_ctx *ctx, const catchhip_candidates *cands,
                                          const uint8_t *draws, int32_t draws_per_probe,
                                          int32_t k, catchhip_probes **out);

/* Statistics of a row table without fetching it (coverage analysis of large
 * designs, catch/coverage_analysis.py:282-335): per universe total_len = sum of
 * (end - start) over its rows (:318-320) and union_len = bases covered by at
 * least one row (:282-302); per set id < num_sets the number of universes it
 * has rows in (probe_map_counts, :255-258, with one universe per sequence).
 * Every set id in the table must be < num_sets when num_sets > 0. */
int catchhip_rows_stats(catchhip_ctx *ctx, const catchhip_rows *rows,
                        int64_t *total_len, int64_t *union_len,
                        int64_t num_sets, int64_t *universes_per_set);

/* Sliding-window depth of a row table without fetching it (csrc/analysis.hip; replaces the per-base loop and the
 * per-window np.average of catch/coverage_analysis.py:336-413).  `rows` is a table from catchhip_cover_ranges (or any
 * table that is not deferred) with one universe per sequence.  Span s is the run of universes [span_first[s],
 * span_first[s + 1]): one genome, its chromosomes concatenated, so windows cross chromosome boundaries as in the
 * reference.  span_first[0 .. nspans] must be non-decreasing within [0, universes of the table].
 *   depth[pos] = rows whose [start, end) holds pos, modulo 2^16 (the reference stores it as uint16, :377)
 *   windows of a span of n bases start at 0, stride, 2 stride, .. < n (:401); one with start + length > n becomes
 *   [n - length, n) (:403-407), and when n < length numpy's slice rule makes that [max(0, 2n - length), n).
 * span_windows[s] receives the number of windows of span s (ceil(n / stride); 0 for an empty span).  With sums ==
 * counts == NULL that is all the call does (no device work): callers size their arrays with it.  Otherwise, for
 * every window of every span in order, sums[] takes the integer sum of the depth over the window's bases and
 * counts[] their number; capacity = room in both, in windows.  The windows past the end of a span repeat one
 * window; all of them are written.  No float arithmetic happens on the device: the average is double(sum) / count
 * on the host, which equals np.average of the uint16 slice (:409-410) because that sum is exact in float64.
 * CATCHHIP_EINVAL: deferred rows, spans out of order or past the universes, window_length or window_stride < 1,
 * capacity too small. */
int catchhip_rows_window_depth(catchhip_ctx *ctx, const catchhip_rows *rows, const int64_t *span_first,
                               int64_t nspans, int64_t window_length, int64_t window_stride,
                               int64_t *span_windows, uint64_t *sums, uint32_t *counts, int64_t capacity);

/* The uncovered regions of a row table without fetching it (csrc/gaps.hip): where a probe set does not reach.
 * `rows` is a table that is neither deferred nor in the direct form (both: CATCHHIP_EINVAL), with one universe per
 * sequence and fewer than 2^32 - 4096 bases, as for catchhip_rows_window_depth.  Rows of different or equal sets may
 * overlap.
 *   depth of a base = the number of rows whose [start, end) holds it, exact in 32 bits (not the uint16 of the
 *   sliding-window report)
 *   region = a maximal run of bases at depth < min_depth inside one universe: two uncovered bases on either side of
 *   a universe boundary belong to two regions, and a universe of length 0 has none
 *   unambiguous count of a region = with `targets`, the number of its bases that are one of A, C, G, T (the rule of
 *   Genome.size(True): N, every other letter and lower case are ambiguous); `targets` must hold one genome per
 *   sequence and have the genome offsets of `rows`, anything else is CATCHHIP_EINVAL.  With targets == NULL the
 *   count is the region's length.
 * A region is reported when its length is >= min_length and its unambiguous count >= min_unambig (0 keeps regions
 * without an unambiguous base).  *out receives a row table of the reported regions in (universe, start) order,
 * to be read with catchhip_rows_fetch -- universe, start and end local to the universe -- whose set_id column
 * carries the unambiguous count (its 32 bits read as unsigned).  That table is a read-out: it is not sorted by set and
 * must not be handed to the calls that take an instance's rows.  *nregions (may be NULL) = its rows; it may be 0,
 * *out is then an empty table, not NULL.  per_universe (may be NULL) receives 3 values per universe, over the
 * reported regions: their number, their bases, the longest.  Integer arithmetic throughout; the result does not
 * depend on the order of the device's atomics.  The device time is left in phase 1 of catchhip_ctx_last_kernel_ms.
 * CATCHHIP_EINVAL: min_depth < 1, min_length < 1, min_unambig < 0, deferred or direct rows, targets of another
 * shape. */
int catchhip_rows_uncovered(catchhip_ctx *ctx, const catchhip_rows *rows, const catchhip_targets *targets,
                            int32_t min_depth, int64_t min_length, int64_t min_unambig, catchhip_rows **out,
                            int64_t *nregions, int64_t *per_universe);

/* ---- target regions: the wanted bases of a coordinate space (csrc/mask.hip) ----
 * A base mask says, for every base of a coordinate space (ngenomes universes of genome_len[u] bases, concatenated as
 * catchhip_rows_from_host lays them out), whether it is WANTED: whether a design has to cover it at all.  The
 * reference has no counterpart (it designs for every base of its genomes).  The n wanted intervals (universe[i],
 * [start[i], end[i]) local to the universe) come in normal form: sorted by (universe, start), 0 <= start < end <=
 * genome_len[universe], and inside a universe every start greater than the end before it (neither overlapping nor
 * touching).  Anything else is CATCHHIP_EINVAL with a message that names the first offending interval, as are
 * 2^32 - 1 bases and more.  n == 0: nothing is wanted.  The bitmap is built word-parallel (a lane per 64 bases, every
 * word stored once; the time does not depend on the intervals' lengths) and wanted_per_universe[ngenomes] (may be
 * NULL) receives the wanted bases of every universe, counted on the device.  Timed as phase 1. */
typedef struct catchhip_basemask catchhip_basemask;
int catchhip_basemask_create(catchhip_ctx *ctx, const int64_t *genome_len, int32_t ngenomes, const int32_t *universe,
                             const int64_t *start, const int64_t *end, int64_t n, catchhip_basemask **out,
                             int64_t *wanted_per_universe);
/* words[(total + 63) / 64]: bit b % 64 of word b / 64 is set iff base b (global) is NOT wanted; the bits behind the
 * last base are set. */
int catchhip_basemask_fetch(catchhip_ctx *ctx, const catchhip_basemask *mask, uint64_t *words);
int catchhip_basemask_destroy(catchhip_basemask *mask);
/* out = every row of `rows` cut into its maximal runs of wanted bases, with the row's set and universe, in the order
 * of `rows`: catchhip_rows_subtract with "covered" = the bases nobody wants.  `rows` as there; the result is sorted
 * and normalised like `rows`, carries gain0 when `rows` does (as catchhip_rows_subtract carries it) and goes to
 * catchhip_setcover_greedy as it is.  *nrows (may be NULL) = its row count; an empty table gives an empty table.
 * CATCHHIP_EINVAL for deferred, direct or grouped rows, a mask over another coordinate space (other universe lengths),
 * 2^32 - 1 target bases and more, 2^31 rows or pieces and more.  Timed as phase 1. */
int catchhip_rows_restrict(catchhip_ctx *ctx, const catchhip_rows *rows, const catchhip_basemask *mask,
                           catchhip_rows **out, int64_t *nrows);
/* catchhip_rows_uncovered over the wanted bases only: a region is a maximal run of WANTED bases at depth < min_depth
 * inside one universe -- an unwanted base ends a run as a covered base does, so two wanted stretches that touch only
 * through unwanted bases give two regions.  Everything else as catchhip_rows_uncovered; CATCHHIP_EINVAL also for a
 * mask over another coordinate space. */
int catchhip_rows_uncovered_within(catchhip_ctx *ctx, const catchhip_rows *rows, const catchhip_targets *targets,
                                   const catchhip_basemask *mask, int32_t min_depth, int64_t min_length,
                                   int64_t min_unambig, catchhip_rows **out, int64_t *nregions,
                                   int64_t *per_universe);

/* Where every set id < num_sets was seen first, on rows from catchhip_cover_scan_first_seen with one universe per
 * sequence: first_universe[s] = the first universe set s has rows in (-1: none) and first_key[s] = the key of the
 * first accepted seed there (catchhip_rows_fetch_first_seen).  Sorting the sets by (first_universe, first_key)
 * gives the order in which catch/coverage_analysis.py:245-250 first meets each probe, i.e. the order of its
 * probe_map_counts. */
int catchhip_rows_first_seen_per_set(catchhip_ctx *ctx, const catchhip_rows *rows, int64_t num_sets,
                                     int32_t *first_universe, uint64_t *first_key);

/* Property checks of a set-cover solution by kernels independent of the solvers (csrc/check.hip), usable at any
 * scale: `picks` are set ids IN THE ORDER they were picked, `rows` the instance's row table (not a deferred one),
 * universe_p per universe or NULL (every universe fully covered).  out5[0] = picks that covered no new position
 * when their turn came (catch/utils/set_cover.py:448-550 only picks a set with a positive gain), out5[1] =
 * universes covered short of |U| - int(|U| - p |U|) (set_cover.py:362-373, U = union of all rows of the universe),
 * out5[2] = pick ids out of range or repeated, out5[3] = bases in the universes, out5[4] = of them covered.
 * A correct solution has out5[0] == out5[1] == out5[2] == 0. */
int catchhip_rows_cover_check(catchhip_ctx *ctx, const catchhip_rows *rows, int64_t num_sets, const int64_t *picks,
                              int64_t npicks, const double *universe_p, int64_t *out5);

/* AdapterFilter._make_votes_across_target_genomes (catch/filter/adapter_filter.py
 * :299-361) on rows from catchhip_cover_scan_first_seen with one universe per
 * sequence: per sequence, in order, the greedy interval schedule over its
 * ranges sorted by end (ties by first-discovery key; catch/utils/interval.py
 * :319-358) gives the scheduled probes an 'A' vote and the other hybridizing
 * probes a 'B' vote, and the sequence's votes are swapped when that makes the
 * sum over all probes of max(A, B) strictly larger; multiplicity[set id] = how
 * many input probes equal that probe (each counts in the sums).  Returns the
 * totals per set id (num_sets must exceed every set id of the table). */
int catchhip_adapter_votes(catchhip_ctx *ctx, const catchhip_rows *rows,
                           int64_t num_sets, const int64_t *multiplicity,
                           int64_t *votes_a, int64_t *votes_b);

#ifdef __cplusplus
}
#endif
#endif /* CATCHHIP_H */
