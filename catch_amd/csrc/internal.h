// Internal declarations shared by the translation units of libcatchhip.so.
// gfx950 (MI355X, CDNA4) only: 64-lane wavefronts are assumed throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/catchhip.h"

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int32_t i32;
typedef int64_t i64;

#define WAVE 64

void chip_set_error(const char *fmt, ...);

#define HIP_TRY(expr)                                                         \
    do {                                                                      \
        hipError_t e__ = (expr);                                              \
        if (e__ != hipSuccess) {                                              \
            chip_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,      \
                           hipGetErrorString(e__));                           \
            return CATCHHIP_EHIP;                                             \
        }                                                                     \
    } while (0)

#define TRY(expr)                                                             \
    do {                                                                      \
        int r__ = (expr);                                                     \
        if (r__ != 0) return r__;                                             \
    } while (0)

#define ARG_CHECK(cond)                                                       \
    do {                                                                      \
        if (!(cond)) {                                                        \
            chip_set_error("%s:%d: invalid argument: %s", __FILE__, __LINE__, \
                           #cond);                                            \
            return CATCHHIP_EINVAL;                                           \
        }                                                                     \
    } while (0)

// Environment switches.  Four are part of the product and read with getenv(): CATCHHIP_TIMING (host-side wall
// times on stderr), CATCHHIP_RCCL_PATH, CATCHHIP_POOL_SOFT_LIMIT_GB, CATCHHIP_GATHER_THREADS (README.md lists them
// with the Python side's).  Everything else is a TEST HOOK -- it forces one of several exact code paths (the
// sequential solver, the fused solver on a large instance, striped tiles ...) so that tests/ and bench.py can
// compare them -- and is only honoured when CATCHHIP_TEST_HOOKS=1 is set (tests/conftest.py and bench.py do).
// A hook exists only while a test, bench.py or a script under tools/ sets it (tests/test_host_logic.py checks), and
// it is read at every decision it takes part in, never cached: a test may set it between two calls.
static inline const char *chip_test_env(const char *name) {
    static const bool on = [] { const char *e = getenv("CATCHHIP_TEST_HOOKS"); return e && atoi(e) != 0; }();
    return on ? getenv(name) : nullptr;
}
// an integer hook: its value, `unset` when it is not set
static inline long long chip_test_env_int(const char *name, long long unset) {
    const char *e = chip_test_env(name);
    return e ? atoll(e) : unset;
}

// Caching device allocator (core.hip): hipMalloc/hipFree cost tens of
// microseconds and hipFree synchronises the device, which would dominate the
// millisecond-scale calls of this library.  Blocks are rounded up to a size
// class and kept on per-device free lists until the process exits; a block is
// only reused by work enqueued later on the context's single stream, after
// the host has observed the previous user's results.
void *chip_pool_alloc(size_t bytes);
// The cache is partitioned by owner (a context): entry points open a PoolScope
// so that blocks are only ever reused on the stream they were used on.
const void *chip_pool_set_owner(const void *owner);
void chip_pool_release_owner(const void *owner);
struct PoolScope {
    const void *prev;
    explicit PoolScope(const void *owner) : prev(chip_pool_set_owner(owner)) {}
    ~PoolScope() { chip_pool_set_owner(prev); }
};
void chip_pool_free(void *p);
// test hook CATCHHIP_POOL_POISON: fills `bytes` at p with the hook's byte (core.hip); the pool calls it at every
// hand-out, and so does every direct hipMalloc whose memory kernels read
void chip_poison_fill(void *p, size_t bytes);
// what the cache may hold (bytes): 0.87 of the device, or CATCHHIP_POOL_SOFT_LIMIT_GB
size_t chip_pool_soft_limit();

// Device buffer owning a pooled region (returned to the pool in the destructor).
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) chip_pool_free((void *)p);
        p = nullptr;
        n = 0;
    }
    int alloc(size_t count) {
        release();
        n = count;
        size_t bytes = (count ? count : 1) * sizeof(T);
        p = (T *)chip_pool_alloc(bytes);
        if (!p) return CATCHHIP_ENOMEM;
        return 0;
    }
    // grow (content not preserved)
    int reserve(size_t count) {
        if (count <= n && p) return 0;
        return alloc(count);
    }
    void swap(DevBuf &o) {
        T *tp = p; p = o.p; o.p = tp;
        size_t tn = n; n = o.n; o.n = tn;
    }
};

enum { PHASE_SCAN = 0, PHASE_ROWS = 1, PHASE_GREEDY = 2, PHASE_NDF = 3, PHASE_GREEDY_ROUNDS = 4, PHASE_VERIFY = 5,
       PHASE_CLAIM = 6, PHASE_VCOUNT = 7, PHASE_POOL = 8, PHASE_PREFILTER = 9, NPHASE = 10 };
#define CHIP_EVX 16   // event pairs for per-launch timing inside a batch of solver rounds (PHASE_CLAIM)

struct catchhip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2 * NPHASE] = {};
    hipEvent_t evx[2 * CHIP_EVX] = {};
    double phase_ms[NPHASE] = {};
    i64 phase_launches[NPHASE] = {};
    i64 counters[8] = {};
    i64 ndf_counters[4] = {};      // last Hamming near-duplicate filter: probes, tables, pairs compared, edges
    i64 solver_levels[2] = {};     // row-parallel solver: gain levels gone through, bands (setcover_flat.inc)
    i64 solver_band_groups = 0;    // row-parallel solver: groups that got band boundaries of their own (1: one row of boundaries)
    i64 solver_counters[4] = {};   // row-parallel solver: records streamed, rows counted again, bitmap words read, owner words looked at
    i64 rows_direct = 0;     // the last catchhip_setcover_filter solved from the bucketed records (catchhip_rows::rows4), no SoA table
    i64 seeds_dropped = 0;   // of counters[1]: work-list entries the seed look-up's anchor-pair filter left empty
    i64 join_counters[4] = {};     // last key-grouped join: hit positions, pairs verified, lane slots of wave-wide runs, tasks of cut runs
    i64 grid_counters[4] = {};     // last catchhip_setcover_grid: scans, derived tables, solves, rows of the e = 0 scan
    // last scan / near-duplicate filter: how often the host found a device buffer too small for what the device counted
    // and ran again at the exact size, or took the slower path (CAPEV_*; catchhip_ctx_last_capacity_events)
    i64 capacity_events[8] = {};
    // pinned staging word(s) for small device->host reads
    u64 *h_pin = nullptr;
    // larger pinned staging area (grown on demand) so that result read-backs are
    // truly asynchronous and one synchronisation collects all of them
    void *h_big = nullptr;
    size_t h_big_bytes = 0;
    // RCCL (optional)
    void *comm = nullptr;
    int nranks = 1, rank = 0;
    int num_cus = 256;
};

enum { CAPEV_SEED_LIST = 0,     // seed-list scan: work list re-run
       CAPEV_GENERAL_SEED = 1,  // general scan, table look-up: work list re-run
       CAPEV_BYTE_JOIN = 2,     // general scan, join of byte hashes: match list re-run
       CAPEV_FAST_HIT = 3,      // tiled scan: hit list re-run
       CAPEV_CUT_LIST = 4,      // general scan: more cut windows than the list holds, every seed extended by bytes
       CAPEV_GIANT_TASKS = 5,   // key-grouped join: more tasks of cut runs than the list holds, the seed-list scan instead
       CAPEV_NDF_EDGES = 6,     // near-duplicate filters, edge-list form: edge list re-run
       NCAPEV = 8 };            // ([7] spare)
static inline void chip_capacity_events_reset(catchhip_ctx *ctx) { memset(ctx->capacity_events, 0, sizeof(ctx->capacity_events)); }

// pinned host scratch of at least `bytes` (contents not preserved on growth)
int chip_pinned_reserve(catchhip_ctx *ctx, size_t bytes);

// small synchronous read-back: `bytes` (at most the 512 of h_pin) from the device to *out, through the pinned words
static inline int chip_read_back(catchhip_ctx *ctx, const void *d, size_t bytes, void *out) {
    HIP_TRY(hipMemcpyAsync(ctx->h_pin, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(out, ctx->h_pin, bytes);
    return 0;
}
static inline int read_count(catchhip_ctx *ctx, const u32 *d, u32 *out) { return chip_read_back(ctx, d, sizeof(u32), out); }

// elapsed time of a phase whose start/stop events were recorded earlier
void chip_phase_collect(catchhip_ctx *ctx, int phase);
// scan + row build with no host synchronisation (seed path only); returns 1
// when the inputs do not qualify (the caller then uses catchhip_cover_scan)
int chip_cover_scan_nosync(catchhip_ctx *ctx, const catchhip_probes *P, const catchhip_targets *T, i32 mismatches,
                           i32 lcf_thres, i32 island, i32 cover_extension, i32 mode, catchhip_rows **out);
// frontier solver on deferred rows; *retry = 1 when the device found the
// deferred scan unusable (overflow, long rows): redo through the synchronous calls
int chip_greedy_deferred(catchhip_ctx *ctx, catchhip_rows *R, i64 num_sets, const i64 *ranks, i64 *out_ids,
                         i64 *n_out, int *retry);
// catchhip_cover_scan for a caller that solves at once (catchhip_setcover_filter): the rows may come back in
// DIRECT form (catchhip_rows::rows4) -- the bucketed records of the row build, no SoA table
int chip_cover_scan_direct(catchhip_ctx *ctx, const catchhip_probes *P, const catchhip_targets *T, i32 mismatches,
                           i32 lcf_thres, i32 island, i32 cover_extension, i32 mode, catchhip_rows **out, i64 *nrows);
// direct rows -> the SoA table (set_id / univ / gs / ge), for the solvers that index four arrays; no-op on SoA rows
int chip_rows_materialise(catchhip_ctx *ctx, catchhip_rows *R);
// catchhip_setcover_greedy on rows of either form (materialises direct rows unless the row-parallel solver takes them)
int chip_setcover_solve(catchhip_ctx *ctx, catchhip_rows *R, i64 num_sets, const i64 *ranks, const double *universe_p,
                        i64 *out_ids, i64 *n_out);

struct catchhip_targets {
    catchhip_ctx *ctx = nullptr;
    i64 total = 0;    // total bases (concatenated)
    i64 nseq = 0;
    i32 ngenomes = 0;
    i64 min_seq_len = 0;
    bool dna5 = false;   // alphabet subset of {A,C,G,T,N}
    bool has_n = false;  // contains a symbol other than A,C,G,T
    DevBuf<u8> bytes;        // raw characters
    DevBuf<u32> seq_off;     // nseq+1, global offsets (u32: total < 2^32)
    DevBuf<i32> seq_genome;  // nseq
    bool has_groups = false;
    DevBuf<i32> seq_group;   // nseq: instance of the sequence's genome (catchhip_targets_set_groups)
    i32 ngroups_set = 0;     // 1 + the largest group number
    // the distinct group numbers, ascending (host and device): a group's place in it is its DENSE number, which the
    // row-parallel solver's per-group band boundaries go by (catchhip_rows::set_group)
    std::vector<i32> h_group_ids;
    DevBuf<i32> group_ids;
    DevBuf<u32> genome_off;  // ngenomes+1 global offset of each genome's first base
    i64 nwords = 0;          // 32-base words per plane (+ padding)
    DevBuf<u32> planes;      // 3 planes, SoA: plane b at planes + b*nwords
    // the same bits word-interleaved, [word] = {plane0, plane1, plane2, 0}: a
    // window of the seed-verify kernel is ONE run of 16-byte words (nwords entries)
    DevBuf<uint4> tq;
    std::vector<i64> h_seq_off;
    std::vector<i32> h_seq_genome;
    std::vector<i64> h_genome_off;
};

struct catchhip_probes {
    catchhip_ctx *ctx = nullptr;
    i64 nprobes = 0;
    i64 total = 0;
    i64 nent = 0;
    i32 k = 0;
    i32 L = 0;            // common probe length, or -1 if lengths differ
    bool dna5 = false;
    bool has_n = false;
    bool pigeonhole = false;  // anchors are exactly {0,k,2k,..,L-k} for every probe
    bool bucket_identity = false;   // bucket_of[p] == p and bucket_set[b] == b (probes from the device front end): no look-ups
    bool sorted_unique = false;   // the caller's anchor entries were sorted by (probe, position), no duplicates
    bool has_groups = false;
    DevBuf<i32> group;       // nprobes: instance of each probe (catchhip_probes_set_groups)
    // seeds per target base seen by earlier seed scans with these probes (sizes the work list)
    mutable double seed_ratio_hint = 0.0;
    i64 max_set_id = 0;
    DevBuf<u8> bytes;
    DevBuf<u32> probe_off;   // nprobes+1
    DevBuf<i32> set_id;      // nprobes
    i64 nbuckets = 0;        // distinct set ids
    DevBuf<u32> bucket_of;   // nprobes: dense rank of the probe's set id (row-table order)
    DevBuf<i32> bucket_set;  // nbuckets: set id of each bucket, ascending
    DevBuf<i32> ent_probe, ent_pos;
    // the same anchors sorted by (probe, position) + first entry of every probe (seed scan)
    DevBuf<u32> sent_probe, sent_pos, ent_ptr;
    i32 pwords = 0;          // 32-base words per probe (ceil(L/32))
    DevBuf<u32> planes;      // [probe][word][4] = planes 0,1,2 + pad per 32-base word
    DevBuf<uint2> w0;        // [probe] word 0 of planes 0/1 (the scan's 32-base filter), masked to L
};

// planes + word-0 image of equal-length DNA probes from p->bytes / p->probe_off (core.hip)
int chip_probes_pack_planes(catchhip_probes *p);

// near-duplicate filters on probes already on the device (ndf.hip): n rows of L
// characters / rows at probe_off[] (>= 16 bytes of slack after the last one);
// keep[] is a host array; d_keep_flags (instead, or nullptr) takes the verdicts as 0/1 words on the device
int chip_ndf_hamming_device(catchhip_ctx *ctx, const u8 *d_rows, i64 n, i32 L, const i32 *positions, i32 ntables,
                            i32 k, i32 dist_thres, u8 *keep, const u32 *d_grp, i64 ngroups, u32 *d_keep_flags = nullptr);
int chip_ndf_minhash_rows(catchhip_ctx *ctx, const u8 *d_rows, i64 n, i64 L, const u32 *d_grp, i64 ngroups, i32 kmer_size,
                          const i64 *ab, i32 ntables, i32 k, double dist_thres, u32 *d_keep_flags);
int chip_ndf_minhash_device(catchhip_ctx *ctx, const u8 *d_rows, const i64 *probe_off, i64 n, const i64 *group_off,
                            i64 ngroups, i32 kmer_size, const i64 *ab, i32 ntables, i32 k, double dist_thres,
                            u8 *keep);

// rows: cover intervals in GLOBAL coordinates of a targets object
struct catchhip_rows {
    catchhip_ctx *ctx = nullptr;
    i64 n = 0;
    i64 total = 0;       // size of the global coordinate space
    i32 ngenomes = 0;
    u32 lmax = 0;        // longest row (bases)
    // Deferred rows (fused scan + solve, never handed to the caller): the scan
    // has not been synchronised, n is only the capacity of the arrays and the
    // facts live on the device: info[0..7] = row-build results (scan.hip "res
    // words": [1] overflow, [2] hits, [4] rows, [5] longest row), info[8..11] =
    // seed counters ([9] seeds), info[12] = seed capacity
    bool deferred = false;
    // the scan's probes / targets carried group numbers (a union of independent instances, catchhip_*_set_groups): its
    // coordinate space is a row of unlike groups, which the row-parallel solver cuts into more, smaller tiles
    bool grouped = false;
    // grouped rows of a merged scan that carry gain0: set_group[s] = dense number (0 .. ngroups - 1: the place of the
    // group number among the targets' distinct ones) of the group of set s, ~0 for a set none of whose probes belongs
    // to a group of the targets (it has no rows); set_group[set_group_n] != 0: some set has probes in several groups
    // (the solver then cuts all sets by one row of boundaries).  set_group_n = 0: not there
    DevBuf<u32> set_group;
    u32 set_group_n = 0, ngroups = 0;
    // cover extension of the merged rows of a cover scan (or of catchhip_rows_extend); -1: anything else (host rows,
    // unmerged ranges, deferred rows) -- catchhip_rows_extend derives only from rows made at 0
    i32 ext = -1;
    DevBuf<u32> info;
    mutable double seed_ratio_seen = 0.0;   // filled by the deferred solve: seeds per target base of the scan
    DevBuf<i32> set_id;
    DevBuf<i32> univ;
    DevBuf<u32> gs, ge;
    // catchhip_cover_scan_first_seen only: per row, the first-discovery key of its (set, universe) group
    DevBuf<unsigned long long> first_key;
    DevBuf<u32> genome_off;  // ngenomes+1
    std::vector<i64> h_genome_off;
    // gain0[s] = total length of set s's rows (the bucketed row build sums a bucket's merged rows on the way):
    // the first round's gains of a full-coverage solve, which then needs no count launch of its own; gain0_n = 0: not there
    DevBuf<u32> gain0;
    u32 gain0_n = 0;
    // DIRECT form (chip_cover_scan_direct; rows4.p != null, the four SoA arrays are empty): the row build's bucket-grouped
    // records {.x start, .y end, .z universe, .w bucket} as bucket_merge left them.  Bucket b owns the slots from
    // bstart[b]; its mcnt[b] merged rows sit at the front of them, in start order, and the stale records behind them
    // keep .w == b -- slot i is a row iff i - bstart[rows4[i].w] < mcnt[rows4[i].w].  slots = the slots to look at
    // (== n when nothing merged: then every slot is a row and nobody tests).  rstart = exclusive scan of mcnt (the
    // row numbers of the SoA form).  The set of bucket b is bucket_set[b], or b itself when bucket_set is null.
    DevBuf<uint4> rows4;
    DevBuf<u32> bstart, mcnt, rstart;
    i64 slots = 0;
    u32 nb = 0;
    const i32 *bucket_set = nullptr;   // (the probes' array: they outlive the filter call the rows live in)
};

// unique candidate probes of a targets object (candidates.hip; the pre-filters of prefilter.hip edit the list)
struct catchhip_candidates {
    catchhip_ctx *ctx = nullptr;
    const catchhip_targets *T = nullptr;   // borrowed: must outlive this object
    i32 L = 0;
    i64 ncand = 0, nuniq = 0;
    DevBuf<u32> upos;   // global start of every unique candidate, first-occurrence order
    DevBuf<u32> mult;   // how many candidates equal each unique one (valid until a near-duplicate filter ran)
    bool grouped = false;   // the targets carry groups: duplicates are only removed inside a group
    i32 ngroups = 0;
    DevBuf<u32> ugrp;   // group of every unique candidate (non-decreasing)
    bool filtered = false;   // a near-duplicate filter replaced the list (multiplicity order, kept ones only)
};
// flag[0..n) (device, 0 / 1; n + 1 words allocated): the unique list becomes the flagged candidates, order kept --
// upos, mult and (grouped) ugrp compacted, nuniq updated (candidates.hip: cand_scan + cand_compact_kernel)
int chip_candidates_keep_flagged(catchhip_ctx *ctx, catchhip_candidates *C, DevBuf<u32> &flag, i64 *nkept);

// The k-mers of a background on the device (background.hip builds it and says what it holds; measure.hip reads it)
struct catchhip_kmer_index {
    int device = 0;
    i32 k = 0;
    u64 n_valid = 0, n_unique = 0;
    u32 P = 8;                       // directory bits
    u64 *codes = nullptr;            // n_unique (at least one word allocated)
    u32 *dir = nullptr;              // 2^P + 1
    // a tolerant index (mismatches = M > 0): codes / dir / P are view 0; view b = 1 .. M is [b - 1] below -- the same
    // codes rotated left by 2 * view_start[b - 1] bits inside their 2k bits, sorted, and a directory of view_P bits
    i32 mismatches = 0;
    u32 view_start[2] = {0, 0};      // s_b: the first character of block b
    u32 view_P[2] = {8, 8};
    u64 *view_codes[2] = {nullptr, nullptr};
    u32 *view_dir[2] = {nullptr, nullptr};
    ~catchhip_kmer_index() {
        if (codes) (void)hipFree(codes);
        if (dir) (void)hipFree(dir);
        for (int b = 0; b < 2; ++b) {
            if (view_codes[b]) (void)hipFree(view_codes[b]);
            if (view_dir[b]) (void)hipFree(view_dir[b]);
        }
    }
};

// MinHash signatures of sequences on the device (cluster.hip; linkage.hip reads them)
struct catchhip_sigs {
    catchhip_ctx *ctx = nullptr;
    u32 nseq = 0, N = 0;
    DevBuf<u32> sig;    // [nseq][N], ascending
    DevBuf<u32> sigT;   // [N][nseq]
    DevBuf<u64> fpT;    // 4,096-bit fingerprints of the signatures, [word][nseq] (catchhip_sigs_neighbors_many, on first use)
    DevBuf<u32> fp_excess;
    bool fp_ready = false;
    // the neighbour graph (catchhip_sigs_graph): rows of g_idx / g_com delimited by g_ptr
    DevBuf<u64> g_ptr;
    DevBuf<u32> g_idx, g_com;
    u64 g_edges = 0;
    bool g_ready = false;
};

// common values met by the N-step merge walk of two ascending N-value lists.
// Branch-free: the three-way comparison of a divergent wavefront would run all
// three paths every step (measured: 28-33 us per row of 6,000 walks, one
// wavefront per CU, whether the values came from L2 or from LDS).
template <typename FA, typename FB> __device__ __forceinline__ u32 walk_common(u32 N, FA a_at, FB b_at) {
    u32 ia = 0, ib = 0, common = 0;
    for (u32 step = 0; step < N; ++step) {
        const u32 act = (ia < N) & (ib < N);           // the reference's loop condition
        const u32 a = a_at(min(ia, N - 1)), b = b_at(min(ib, N - 1));
        const u32 lt = act & (a < b), gt = act & (a > b), eq = act & (a == b);
        ia += lt | eq;
        ib += gt | eq;
        common += eq;
    }
    return common;
}

// ---- timing helpers -----------------------------------------------------
struct PhaseTimer {
    catchhip_ctx *c;
    int phase;
    bool stopped = false;
    // keep = true continues a phase that was already timed once in this call:
    // finish_add() then adds to its time instead of replacing it
    PhaseTimer(catchhip_ctx *ctx, int ph, bool keep = false) : c(ctx), phase(ph) {
        if (keep) (void)hipEventRecord(c->ev[2 * phase], c->stream);
        else restart();
    }
    void restart() {
        stopped = false;
        c->phase_launches[phase] = 0;
        c->phase_ms[phase] = 0.0;
        (void)hipEventRecord(c->ev[2 * phase], c->stream);
    }
    void launch(i64 k = 1) { c->phase_launches[phase] += k; }
    // records the stop event (first call wins); finish() reads it after a sync
    void stop() {
        if (stopped) return;
        stopped = true;
        (void)hipEventRecord(c->ev[2 * phase + 1], c->stream);
    }
    void finish() {
        float ms = 0.f;
        stop();
        (void)hipEventSynchronize(c->ev[2 * phase + 1]);
        // (timing is best effort: a failing query leaves the phase's time as it was)
        if (hipEventElapsedTime(&ms, c->ev[2 * phase], c->ev[2 * phase + 1]) == hipSuccess)
            c->phase_ms[phase] = ms;
    }
    void finish_add() {
        const double before = c->phase_ms[phase];
        finish();
        c->phase_ms[phase] += before;
    }
};

// ---- the wanted bases of a coordinate space (mask.hip; catchhip_rows_restrict, catchhip_rows_uncovered_within) ---
struct catchhip_basemask {
    catchhip_ctx *ctx = nullptr;
    i64 total = 0;       // size of the coordinate space (universes concatenated, as catchhip_rows_from_host lays them out)
    i32 ngenomes = 0;
    std::vector<i64> h_genome_off;
    // bit b set = base b is not wanted; chip_cut_bitmap_words(total) words (rows_host.h: chip_rows_cut reads it as it
    // reads its own), the bits at and beyond `total` set
    DevBuf<unsigned long long> unwanted;
};

// ---- device primitives (primitives.hip) ---------------------------------
// exclusive prefix sum of n u32 values (in place allowed: out may equal in);
// if total != nullptr, *total (device u64) receives the grand total.
int chip_exclusive_scan_u32(catchhip_ctx *ctx, const u32 *in, u32 *out, i64 n,
                            DevBuf<u32> &tmp);
// the scratch that scan needs for up to n values, reserved in tmp ahead of time
int chip_exclusive_scan_reserve(DevBuf<u32> &tmp, i64 n);
// Stable LSD radix sort of (u64 key, u32 value) pairs on bits [first_bit, first_bit + key_bits).
// Result ends in keys/vals (the alt buffers are scratch of the same size).
int chip_radix_sort_pairs(catchhip_ctx *ctx, DevBuf<u64> &keys, DevBuf<u64> &keys_alt,
                          DevBuf<u32> &vals, DevBuf<u32> &vals_alt, i64 n, int key_bits, int first_bit = 0);
// nseg segments of n keys each, side by side, every segment sorted on its own (one set of launches for all)
int chip_radix_sort_pairs_segments(catchhip_ctx *ctx, DevBuf<u64> &keys, DevBuf<u64> &keys_alt, DevBuf<u32> &vals,
                                   DevBuf<u32> &vals_alt, i64 n, i64 nseg, int key_bits, int first_bit = 0);

// v mod (2^31 - 1) for v < 2^63 without a 64-bit division: 2^31 = 1 (mod p),
// so the 31-bit digits of v add up (two folds leave at most p + 1)
__host__ __device__ static inline u32 mod_mersenne31(u64 v) {
    const u64 P = 0x7fffffffull;
    u64 t = (v & P) + (v >> 31);      // < 2^33
    t = (t & P) + (t >> 31);          // <= p + 3
    return (u32)(t >= P ? t - P : t);
}

// CPython <= 3.10 hash(str) of `len` ASCII characters under PYTHONHASHSEED=0: SipHash-2-4 with an all-zero
// key (PEP 456, Python/pyhash.c).  The reference hashes Probe objects by hash(seq_str) (catch/probe.py:
// 324-329): its sets of probes iterate in an order that follows from these values.
__host__ __device__ static inline long long chip_pyhash_seed0(const u8 *src, int len) {
    u64 v0 = 0x736f6d6570736575ull, v1 = 0x646f72616e646f6dull, v2 = 0x6c7967656e657261ull, v3 = 0x7465646279746573ull;
#define CHIP_SIPROUND do { \
    v0 += v1; v1 = (v1 << 13) | (v1 >> 51); v1 ^= v0; v0 = (v0 << 32) | (v0 >> 32); \
    v2 += v3; v3 = (v3 << 16) | (v3 >> 48); v3 ^= v2; \
    v0 += v3; v3 = (v3 << 21) | (v3 >> 43); v3 ^= v0; \
    v2 += v1; v1 = (v1 << 17) | (v1 >> 47); v1 ^= v2; v2 = (v2 << 32) | (v2 >> 32); } while (0)
    u64 b = (u64)len << 56;
    int n = len;
    const u8 *p = src;
    while (n >= 8) {
        u64 mi = 0;
        for (int i = 0; i < 8; ++i) mi |= (u64)p[i] << (8 * i);
        v3 ^= mi; CHIP_SIPROUND; CHIP_SIPROUND; v0 ^= mi;
        p += 8; n -= 8;
    }
    u64 t = 0;
    for (int i = 0; i < n; ++i) t |= (u64)p[i] << (8 * i);
    b |= t;
    v3 ^= b; CHIP_SIPROUND; CHIP_SIPROUND; v0 ^= b;
    v2 ^= 0xff; CHIP_SIPROUND; CHIP_SIPROUND; CHIP_SIPROUND; CHIP_SIPROUND;
#undef CHIP_SIPROUND
    long long x = (long long)((v0 ^ v1) ^ (v2 ^ v3));
    if (x == -1) x = -2;
    return x;
}
// order[] = the indices 0..n-1 in the order a CPython set iterates n distinct keys with these hashes
// after they were added in index order (core.hip)
void chip_pyset_order(const i64 *hash, i64 n, i64 *order);

// Body of a function that picks the instance of a kernel template for a probe of nw 32-base words (host side):
// returns KERNEL<nw, further template arguments...> for nw in 1..MAX (MAX is 7 or 8), nullptr for any other nw.
#define PICK_NW_CASES_7(KERNEL, ...)                                                                          \
    case 1: return KERNEL<1, ##__VA_ARGS__>; case 2: return KERNEL<2, ##__VA_ARGS__>;                         \
    case 3: return KERNEL<3, ##__VA_ARGS__>; case 4: return KERNEL<4, ##__VA_ARGS__>;                         \
    case 5: return KERNEL<5, ##__VA_ARGS__>; case 6: return KERNEL<6, ##__VA_ARGS__>;                         \
    case 7: return KERNEL<7, ##__VA_ARGS__>;
#define PICK_NW_CASES_8(KERNEL, ...) PICK_NW_CASES_7(KERNEL, ##__VA_ARGS__) case 8: return KERNEL<8, ##__VA_ARGS__>;
#define PICK_NW(MAX, nw, KERNEL, ...)                                                                         \
    switch (nw) { PICK_NW_CASES_##MAX(KERNEL, ##__VA_ARGS__) }                                                \
    return nullptr

static inline int ceil_log2_u64(u64 x) {
    int b = 0;
    while (b < 64 && ((u64)1 << b) < x) ++b;
    return b;
}
static inline i64 div_up(i64 a, i64 b) { return (a + b - 1) / b; }
