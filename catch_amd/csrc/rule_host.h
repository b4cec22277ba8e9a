// What the entry points of the candidate rules share on the host (prefilter.hip, thermo.hip, structure.hip,
// background.hip, measure.hip): the launch plans, the totals' read-back, the preamble and the tail.  stage.h and
// planes.h hold the device side.
#pragma once
#include <algorithm>

#include "internal.h"
#include "stage.h"

#define POLYA_LDS_BUDGET 65536u

// ---- rows (stage.h) -------------------------------------------------------------------------------------------------
// A row in LDS runs from the 16-byte boundary below its start (<= 15 bytes before it) to its end: nchunk 16-byte
// chunks, at an odd pitch of dwords.  Behind the rows lie row_extra bytes per row (a multiple of 4), then wg_extra bytes
// once per workgroup, the latter aligned to tail_align bytes (4 or 8; 8 costs 4 bytes of the budget for the rounding).
// As many of 256 / 128 / 64 rows as fit the budget; when 64 do not, or the byte array is not 16-byte aligned, the rows
// are not staged: 256 threads, no row region, the extras alone.
struct RowPlan {
    u32 rows, nchunk, pitch_dw;
    bool stage;
    u32 extra_off_dw;                // the per-row extras
    u32 tail_off_dw;                 // the per-workgroup extras
    size_t lds_bytes;
};
static inline RowPlan row_plan(u32 L, size_t row_extra, size_t wg_extra, u32 tail_align, bool bytes_aligned16) {
    RowPlan p;
    p.nchunk = (L + 15u + 15u) / 16u;
    p.pitch_dw = 4u * p.nchunk + 1u;
    const size_t row_bytes = (size_t)p.pitch_dw * 4, pad = tail_align > 4u ? 4u : 0u;
    p.rows = 256;
    while (p.rows > 64 && p.rows * (row_bytes + row_extra) + wg_extra + pad > POLYA_LDS_BUDGET) p.rows >>= 1;
    p.stage = p.rows * (row_bytes + row_extra) + wg_extra + pad <= POLYA_LDS_BUDGET && bytes_aligned16;
    if (!p.stage) p.rows = 256;
    p.extra_off_dw = p.stage ? p.rows * p.pitch_dw : 0u;
    const u32 a = tail_align / 4u;
    p.tail_off_dw = (p.extra_off_dw + p.rows * (u32)(row_extra / 4) + a - 1u) / a * a;
    p.lds_bytes = (size_t)p.tail_off_dw * 4 + wg_extra;
    return p;
}

// the plan for a candidate list, and what a row kernel's launch takes from the two
static inline bool rows_aligned(const catchhip_candidates *C) { return ((uintptr_t)C->T->bytes.p & 15u) == 0; }
static inline dim3 row_grid(const catchhip_candidates *C, const RowPlan &p) {
    return dim3((unsigned)div_up(C->nuniq, p.rows));
}
static inline RowArgs row_args(const catchhip_candidates *C, const RowPlan &p) {
    return RowArgs{(const u8 *)C->T->bytes.p, (const u32 *)C->upos.p, (const u32 *)C->mult.p, (u32)C->nuniq, (u32)C->L,
                   p.nchunk, p.pitch_dw, p.extra_off_dw};
}

// ---- planes (planes.h) ------------------------------------------------------------------------------------------------
// 6 W + 7 words per candidate (three planes, three reversed ones between zero words, odd pitch), W = ceil(L / 32),
// and behind the planes of a workgroup tail_bytes aligned as above.  As many of 256 / 128 / 64 candidates as fit the
// budget; when 64 do not, the planes go to global memory: 256 threads, the tail alone in LDS.
struct PlanePlan {
    u32 W, rows;
    bool lds_planes;
    size_t cand_bytes;
    u32 tail_off_dw;
    size_t lds_bytes;
};
static inline PlanePlan plane_plan(u32 L, size_t tail_bytes, u32 tail_align) {
    PlanePlan p;
    p.W = (L + 31u) / 32u;
    p.cand_bytes = (size_t)(6u * p.W + 7u) * 4;
    const size_t pad = tail_align > 4u ? 4u : 0u;
    p.rows = 256;
    while (p.rows > 64 && p.rows * p.cand_bytes + pad + tail_bytes > POLYA_LDS_BUDGET) p.rows >>= 1;
    p.lds_planes = p.rows * p.cand_bytes + pad + tail_bytes <= POLYA_LDS_BUDGET;
    if (!p.lds_planes) p.rows = 256;
    const size_t a = tail_align / 4u;
    p.tail_off_dw = p.lds_planes ? (u32)((p.rows * p.cand_bytes / 4 + a - 1) / a * a) : 0u;
    p.lds_bytes = (size_t)p.tail_off_dw * 4 + tail_bytes;
    return p;
}

// Planes in global memory: launch(first, end, planes) over the n candidates, as many per launch as the plane buffer
// holds (a multiple of the workgroup of 256).  CATCHHIP_STRUCT_PLANE_BYTES, a test hook, shrinks the buffer so that a
// small list takes several launches.  launch() returns after its hipLaunchKernelGGL; the errors are collected here.
#define RULE_GLOBAL_PLANE_BYTES ((size_t)256 << 20)
template <typename F>
static int launch_over_plane_chunks(catchhip_ctx *ctx, u32 n, size_t cand_bytes, F launch) {
    const size_t budget = (size_t)chip_test_env_int("CATCHHIP_STRUCT_PLANE_BYTES", (long long)RULE_GLOBAL_PLANE_BYTES);
    u32 per = (u32)std::min<size_t>(budget / cand_bytes, (size_t)n);
    per = std::max(256u, (per + 255u) & ~255u);
    DevBuf<u32> planes;
    TRY(planes.alloc((size_t)per * (cand_bytes / 4)));
    for (u32 first = 0; first < n; first += per) {
        launch(first, (u32)std::min<u64>((u64)first + per, n), planes.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));               // (the plane buffer goes back to the pool on return)
    return 0;
}

// ---- totals (stage.h: totals_slot) --------------------------------------------------------------------------------------
// `slots` zeroed copies of a family's totals on the device, slot_words 64-bit words apart, and their sum on the host.
struct SlotTotals {
    DevBuf<u64> d;
    u32 slots = 0, slot_words = 0;
    size_t bytes() const { return sizeof(u64) * slots * slot_words; }
    int init(catchhip_ctx *ctx, u32 nslots, u32 nslot_words) {
        slots = nslots;
        slot_words = nslot_words;
        TRY(d.alloc((size_t)slots * slot_words));
        TRY(chip_pinned_reserve(ctx, bytes()));
        HIP_TRY(hipMemsetAsync(d.p, 0, bytes(), ctx->stream));
        return 0;
    }
    // out[0 .. nwords) = the first nwords words summed over the copies; synchronises the stream
    int read(catchhip_ctx *ctx, u32 nwords, u64 *out) {
        HIP_TRY(hipMemcpyAsync(ctx->h_big, d.p, bytes(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        memset(out, 0, sizeof(u64) * nwords);
        for (u32 slot = 0; slot < slots; ++slot) {
            const u64 *w = (const u64 *)ctx->h_big + (size_t)slot * slot_words;
            for (u32 k = 0; k < nwords; ++k) out[k] += w[k];
        }
        return 0;
    }
};

// ---- the entry points ---------------------------------------------------------------------------------------------------
// An entry point checks its own arguments (ARG_CHECK names its file, line and condition), then refuses a filtered list
// here: `who` is the entry point as its messages name it, `what` the rule as the message about the order of the
// filters names it.  Its own refusals follow, then `PoolScope pool_scope(ctx);` and rule_begin.
static inline int rule_refuse_filtered(const catchhip_candidates *C, const char *who, const char *what) {
    if (!C->filtered) return 0;
    chip_set_error("%s: a near-duplicate filter was already applied (the %s comes first)", who, what);
    return CATCHHIP_EINVAL;
}
// the device, and the count that a call which drops nothing reports (nkept may be null)
static inline int rule_begin(catchhip_ctx *ctx, const catchhip_candidates *C, i64 *nkept) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (nkept) *nkept = C->nuniq;
    return 0;
}

// the tail of a rule that drops: the flagged candidates stay
static inline int rule_keep(catchhip_ctx *ctx, catchhip_candidates *C, bool dropped_any, DevBuf<u32> &flag, i64 *nkept) {
    if (!dropped_any) return 0;                               // nothing dropped (or not filtering): the list stands
    return chip_candidates_keep_flagged(ctx, C, flag, nkept);
}
