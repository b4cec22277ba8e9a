// What the entry points that derive a row table from a row table share on the host (subtract.hip, mask.hip, depth.hip,
// prune.hip, gaps.hip, union.hip): a new table over a known coordinate space, the refusals, the scope of a derived
// table, the cut bitmap and the counters' read-back.  spans.h holds the device side.
// An entry checks its own arguments first, in its own order (ARG_CHECK names its file, line and condition), then
// `PoolScope pool_scope(ctx);`, the device, and DerivedRows.
#pragma once
#include "internal.h"

// the four SoA arrays of n rows
static inline int chip_rows_alloc_soa(catchhip_rows *R, size_t n) {
    TRY(R->set_id.alloc(n));
    TRY(R->univ.alloc(n));
    TRY(R->gs.alloc(n));
    TRY(R->ge.alloc(n));
    return 0;
}
// an empty rows object over a coordinate space that is on the device already (a targets object's, or other rows'):
// the host facts, and genome_off copied on the context's stream.  Call under the caller's PoolScope, device set.
static inline int chip_rows_new(catchhip_ctx *ctx, i64 total, i32 ngenomes, const std::vector<i64> &h_genome_off,
                                const u32 *d_genome_off, bool grouped, std::unique_ptr<catchhip_rows> &R) {
    R.reset(new catchhip_rows());
    R->ctx = ctx;
    R->total = total;
    R->ngenomes = ngenomes;
    R->h_genome_off = h_genome_off;
    R->grouped = grouped;
    TRY(R->genome_off.alloc((size_t)ngenomes + 1));
    HIP_TRY(hipMemcpyAsync(R->genome_off.p, d_genome_off, sizeof(u32) * ((size_t)ngenomes + 1), hipMemcpyDeviceToDevice,
                           ctx->stream));
    return 0;
}

// ---- the refusals ---------------------------------------------------------------------------------------------------
// `who` is the entry as its messages name it, `which` the table ("the rows", "the covered rows", ...).
// The form: deferred rows, rows in the direct form and, unless grouped_ok, rows with group numbers are refused
static inline int chip_rows_form_check(const catchhip_rows *R, const char *who, const char *which, bool grouped_ok = false) {
    const char *what = R->deferred ? "are deferred rows (a fused scan that was never synchronised)"
                       : R->rows4.p ? "are in the direct form of the fused filter, not a row table"
                       : (R->grouped && !grouped_ok)
                           ? "come from a scan with group numbers (a union of instances), which is not supported" : nullptr;
    if (!what) return 0;
    chip_set_error("%s: %s %s", who, which, what);
    return CATCHHIP_EINVAL;
}
// The limits of 32-bit coordinates and row numbers: a space of `total` bases, tables of na and nb rows
static inline int chip_rows_limits_check(const char *who, i64 total, i64 na, i64 nb = 0) {
    const char *what = total >= ((i64)1 << 32) - 1 ? "more than 2^32 - 2 target bases"
                       : (na >= ((i64)1 << 31) || nb >= ((i64)1 << 31)) ? "too many rows" : nullptr;
    if (!what) return 0;
    chip_set_error("%s: %s", who, what);
    return CATCHHIP_EINVAL;
}
// The coordinate space: X (rows, a mask or targets) lies over the universes of R0, base for base
template <typename X> static inline bool chip_same_space(const X *x, const catchhip_rows *R0) {
    return x->total == R0->total && x->ngenomes == R0->ngenomes && x->h_genome_off == R0->h_genome_off;
}
// ... `phrase` says what is wrong with x, as in "the mask is not over the coordinate space of the rows"
template <typename X>
static inline int chip_space_check(const X *x, const catchhip_rows *R0, const char *who, const char *phrase) {
    if (chip_same_space(x, R0)) return 0;
    chip_set_error("%s: %s (%lld bases in %d universes against %lld in %d)", who, phrase, (long long)x->total,
                   (int)x->ngenomes, (long long)R0->total, (int)R0->ngenomes);
    return CATCHHIP_EINVAL;
}
// ... and targets have to be one genome per sequence on top of that
static inline int chip_targets_space_check(const catchhip_targets *T, const catchhip_rows *R0, const char *who) {
    if (T->nseq == (i64)T->ngenomes && chip_same_space(T, R0)) return 0;
    chip_set_error("%s: the targets (%lld bases, %lld sequences in %d genomes) are not one genome per "
                   "sequence over the coordinate space of the rows (%lld bases in %d universes)", who,
                   (long long)T->total, (long long)T->nseq, (int)T->ngenomes, (long long)R0->total, (int)R0->ngenomes);
    return CATCHHIP_EINVAL;
}

// ---- rows cut by a bitmap of bases (subtract.hip) -------------------------------------------------------------------
// a copy of the SoA table R0 (with its gain0 and lmax) into R, made by chip_rows_new over the same coordinate space
int chip_rows_copy(catchhip_ctx *ctx, const catchhip_rows *R0, catchhip_rows *R);
// every row of R0 (non-empty, passed chip_rows_form_check, fewer than 2^31 rows) cut into its maximal runs of bases
// whose bit in bm is clear (chip_cut_bitmap's words); the rows of the sets with skip[set] != 0 (set < nskip; skip may be
// null) are left out whole.  Order and normal form of R0 are kept; R gets n, lmax and, when R0 has it, gain0.  tm: the
// caller's running timer (its launches are counted and its stop event recorded here).
int chip_rows_cut(catchhip_ctx *ctx, const catchhip_rows *R0, const unsigned long long *bm, const u8 *skip, u32 nskip,
                  catchhip_rows *R, PhaseTimer &tm, const char *who);
// the words of a bitmap that chip_rows_cut reads, for a space of `total` bases (catchhip_basemask::unwanted has as many)
static inline size_t chip_cut_bitmap_words(i64 total) { return (size_t)(total / 64 + 2) + 8; }
static inline int chip_cut_bitmap(catchhip_ctx *ctx, i64 total, bool zeroed, DevBuf<unsigned long long> &bm) {
    const size_t nwords = chip_cut_bitmap_words(total);
    TRY(bm.alloc(nwords));
    if (zeroed) HIP_TRY(hipMemsetAsync(bm.p, 0, sizeof(unsigned long long) * nwords, ctx->stream));
    return 0;
}

// ---- depth per base from a pick list (depth.hip) --------------------------------------------------------------------
// the refusals catchhip_rows_below_depth, _prune and _pick_gains share: depth < 1, rows chip_rows_form_check refuses,
// chip_rows_limits_check, more picks than sets
int chip_depth_check(const catchhip_rows *R0, i64 num_sets, i64 npicks, i32 depth, const char *who);
// The pick table of the host array picks[0..npicks), npicks > 0: rank[set] = position of the set's pick (CHIP_NOT_PICKED:
// none), picked[set] = 1 as a byte (what chip_rows_cut's kernels index per row), num_sets of each; d_picks = the picks
// on the device.  CATCHHIP_EINVAL ("<who>: a pick ...") for an id outside [0, num_sets) or given twice.
#define CHIP_NOT_PICKED 0xffffffffu
int chip_depth_marks(catchhip_ctx *ctx, const i64 *picks, i64 npicks, i64 num_sets, DevBuf<i64> &d_picks,
                     DevBuf<u32> &rank, DevBuf<u8> &picked, PhaseTimer &tm, const char *who);
// the rows of R (those of the sets with picked[set] != 0, set < num_sets; picked null: all) marked on the difference
// array d by span_mark_diff: one launch, none for an empty table; returns their number
i64 chip_depth_diff(catchhip_ctx *ctx, const catchhip_rows *R, const u8 *picked, u32 num_sets, u32 *d);
// d[b + 1] = depth of base b = the rows of R0's picked sets over it (picked null: all rows), plus the rows of F over it
// (F may be null; otherwise any table over R0's coordinate space, every row counts).  d gets total + 2 entries; tmp =
// the scan's scratch.
int chip_depth_array(catchhip_ctx *ctx, const catchhip_rows *R0, const u8 *picked, u32 num_sets, const catchhip_rows *F,
                     DevBuf<u32> &d, DevBuf<u32> &tmp, PhaseTimer &tm);
// bit b of bm = d[b + 1] >= k (bm: total / 64 + 1 words at least, zeroed by the caller); reached[u] (device, zeroed
// by the caller; may be null) += the bits of universe u
int chip_depth_bitmap(catchhip_ctx *ctx, const u32 *d, u64 total, u32 k, const u32 *genome_off, u32 ng,
                      unsigned long long *bm, unsigned long long *reached, PhaseTimer &tm);

// ---- read-back ------------------------------------------------------------------------------------------------------
// out[0 .. n) = n 64-bit counters of the device, through the pinned staging buffer (out null or n = 0: nothing is
// fetched); synchronises the stream either way
static inline int chip_fetch_counters(catchhip_ctx *ctx, const unsigned long long *d, size_t n, i64 *out) {
    if (out && n) {
        TRY(chip_pinned_reserve(ctx, sizeof(unsigned long long) * n));
        HIP_TRY(hipMemcpyAsync(ctx->h_big, d, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; out && k < n; ++k) out[k] = (i64)((const unsigned long long *)ctx->h_big)[k];
    return 0;
}

// ---- the scope of a derived table -----------------------------------------------------------------------------------
// R = an empty table over R0's coordinate space (ext = -1) and the running PHASE_ROWS timer, started behind the copy of
// genome_off.  `DerivedRows D(ctx, R0); TRY(D.err);`, the entry's launches on D.tm, then `return D.finish(out, nrows);`
struct DerivedRows {
    catchhip_ctx *ctx;
    std::unique_ptr<catchhip_rows> R;
    int err;
    PhaseTimer tm;
    DerivedRows(catchhip_ctx *c, const catchhip_rows *R0)
        : ctx(c), err(chip_rows_new(c, R0->total, R0->ngenomes, R0->h_genome_off, R0->genome_off.p, false, R)),
          tm(c, PHASE_ROWS) {
        if (!err) R->ext = -1;
    }
    // nothing to compute: R = a copy of src, or stays empty (src null or empty: genome_off is on its way, wait for it)
    int copy_of(const catchhip_rows *src) {
        if (src && src->n) return chip_rows_copy(ctx, src, R.get());
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return 0;
    }
    int finish(catchhip_rows **out, i64 *nrows) {
        tm.finish();
        if (nrows) *nrows = R->n;
        *out = R.release();
        return 0;
    }
};
