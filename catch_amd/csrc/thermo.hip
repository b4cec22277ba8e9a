// Melting temperature of every candidate under the nearest-neighbour model (not in the reference;
// catch_amd/filter/tm_filter.py defines the rule in integers and is its oracle), on the device's candidate list, before
// the near-duplicate filter and the set cover like the pre-filters of prefilter.hip.
//
// tm_flag_kernel: one thread per unique candidate, one pass over its L bytes, the rows staged (stage.h).  Per byte one
// look-up of the dinucleotide (previous byte, this byte) in the 16-entry table, which lies in LDS, 16 dwords behind the
// staged rows; the sums and the finish are stage.h's TmSums.
// Counting: behind the table, TM_WORDS 64-bit counters per workgroup -- the 128 bins of whole degrees, then "below" and
// "above".  The threads add their multiplicities to the bins with LDS atomics (exact u64 sums; Tm piles into about 15
// neighbouring bins, which are different banks, and adds to one bin queue in LDS for a few cycles, not in L2); "below"
// and "above" are two addresses for most of the threads of a filtering call, so they are summed over the wave first
// and added once per wave (8.9 M candidates, a range that drops 2 in 3: 0.656 ms; 0.709 with every thread adding).
// After a barrier the counters go to one of TM_SLOTS copies in global memory (stage.h: the totals), chosen by the
// workgroup's number, so that the 35,000 workgroups of 8.9 M candidates do not queue on the same 15 lines.  A copy is
// TM_SLOT_WORDS = 144 words, 9 whole lines.  No thread returns before the barrier.  FILTER = false writes no flag and
// HIST = false touches no bin.
#include "internal.h"
#include "wave.h"
#include "stage.h"
#include "rule_host.h"

#define TM_BINS 128u
#define TM_WORDS 130u                // the bins, below, above
#define TM_SLOTS 64u
#define TM_SLOT_WORDS 144u
#define TM_EXTRA_BYTES (TM_TABLE_DW * 4u + TM_WORDS * 8u)       // behind the rows: 1,104 bytes per workgroup

template <bool STAGE, bool FILTER, bool HIST>
__global__ void __launch_bounds__(256)
tm_flag_kernel(const u8 *__restrict__ bytes, const u32 *__restrict__ upos, const u32 *__restrict__ mult, u32 n, u32 L,
               i64 q, i64 offset_c, i64 lo_c, i64 hi_c, u32 nchunk, u32 pitch_dw, u32 extra_off_dw,
               u32 *__restrict__ flag, u64 *__restrict__ totals) {
    extern __shared__ u32 tm_lds[];
    // (the row arguments one by one, in this order, and the struct made here: as ONE struct argument they moved the
    // others, the scalar loads were cut differently and the kernel ran 0.3 % slower -- DESIGN.md, round 13)
    const RowArgs a = {bytes, upos, mult, n, L, nchunk, pitch_dw, extra_off_dw};
    const u32 rows = blockDim.x, r = threadIdx.x;
    const u32 i = blockIdx.x * rows + r;
    u32 *tbl = tm_lds + a.extra_off_dw;                                             // (extra_off_dw is even: 8-byte aligned)
    unsigned long long *cnt = (unsigned long long *)(tbl + TM_TABLE_DW);
    TmSums::load_table(tbl);
    for (u32 t = r; t < TM_WORDS; t += rows) cnt[t] = 0;
    if (STAGE) stage_rows(a, tm_lds);                                               // (ends with a barrier)
    else __syncthreads();
    u64 t_below = 0, t_above = 0;
    if (i < a.n) {                                            // (no early return: the wave sums and the barrier below)
        const u8 *p = row_ptr<STAGE>(a, tm_lds, i);
        TmSums sums;
        for (u32 j = 0; j < a.L; ++j) {
            const u8 c = p[j];
            const bool b = is_base(c);
            const u32 code = base_code(c);
            sums.step(tbl, code, b);
        }
        const i64 tm_c = sums.tm_c(p[0], p[a.L - 1], q, offset_c);
        const u32 m = a.mult[i];
        if (HIST) {
            const i64 d = tm_c / 100;                         // (tm_c >= 0 where it matters: below 0 is bin 0)
            const u32 bin = tm_c < 0 ? 0u : d > (i64)(TM_BINS - 1u) ? TM_BINS - 1u : (u32)d;
            atomicAdd(cnt + bin, (unsigned long long)m);
        }
        if (FILTER) {
            const bool below = tm_c < lo_c, above = tm_c > hi_c;
            flag[i] = (below || above) ? 0u : 1u;
            t_below = below ? m : 0u;
            t_above = above ? m : 0u;
        }
    }
    if (FILTER) totals_add_per_wave(cnt + TM_BINS, t_below, t_above);
    __syncthreads();
    totals_flush(cnt, TM_WORDS, totals_slot(totals, TM_SLOTS, TM_SLOT_WORDS));
}

typedef decltype(&tm_flag_kernel<false, false, true>) tm_fn;
static tm_fn tm_instance(bool stage, bool filter, bool hist) {            // (filter || hist)
    static const tm_fn table[2][3] = {
        {tm_flag_kernel<false, false, true>, tm_flag_kernel<false, true, false>, tm_flag_kernel<false, true, true>},
        {tm_flag_kernel<true, false, true>, tm_flag_kernel<true, true, false>, tm_flag_kernel<true, true, true>}};
    return table[stage ? 1 : 0][filter ? (hist ? 2 : 1) : 0];
}

extern "C" int catchhip_candidates_drop_tm(catchhip_ctx *ctx, catchhip_candidates *C, i64 q, i32 offset_c, i32 filter_on,
                                           i32 lo_c, i32 hi_c, i64 dropped[3], u64 hist[128], i64 *nkept) {
    ARG_CHECK(ctx && C && C->ctx == ctx);
    TRY(rule_refuse_filtered(C, "candidates_drop_tm", "Tm filter"));
    if (q > -8200) {
        chip_set_error("candidates_drop_tm: q must be <= -8200, so that 100 E + q stays negative (got %lld)", (long long)q);
        return CATCHHIP_EINVAL;
    }
    if (filter_on && lo_c > hi_c) {
        chip_set_error("candidates_drop_tm: lo_c exceeds hi_c (got %d, %d)", (int)lo_c, (int)hi_c);
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    TRY(rule_begin(ctx, C, nkept));
    if (dropped) dropped[0] = dropped[1] = dropped[2] = 0;
    if (hist) memset(hist, 0, sizeof(u64) * TM_BINS);
    if (C->nuniq == 0 || C->L < 2 || !(filter_on || hist)) return 0;
    DevBuf<u32> flag;
    SlotTotals totals;
    if (filter_on) TRY(flag.alloc((size_t)C->nuniq + 1));
    TRY(totals.init(ctx, TM_SLOTS, TM_SLOT_WORDS));
    PhaseTimer tm(ctx, PHASE_PREFILTER);
    const RowPlan plan = row_plan((u32)C->L, 0, TM_EXTRA_BYTES, 4, rows_aligned(C));
    const RowArgs a = row_args(C, plan);                      // (the order below is the kernel's)
    hipLaunchKernelGGL(tm_instance(plan.stage, filter_on != 0, hist != nullptr), row_grid(C, plan), dim3(plan.rows),
                       plan.lds_bytes, ctx->stream, a.bytes, a.upos, a.mult, a.n, a.L, q, (i64)offset_c,
                       (i64)(filter_on ? lo_c : 0), (i64)(filter_on ? hi_c : 0), a.nchunk, a.pitch_dw, a.extra_off_dw,
                       flag.p, totals.d.p);
    HIP_TRY(hipGetLastError());
    tm.launch();
    tm.stop();
    u64 h[TM_WORDS];
    TRY(totals.read(ctx, TM_WORDS, h));
    tm.finish();
    if (hist) memcpy(hist, h, sizeof(u64) * TM_BINS);
    const u64 below = h[TM_BINS], above = h[TM_BINS + 1u];
    if (dropped) { dropped[0] = (i64)below; dropped[1] = (i64)above; dropped[2] = (i64)(below + above); }
    return rule_keep(ctx, C, below + above != 0, flag, nkept);
}
