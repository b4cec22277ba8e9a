// Melting temperature of every candidate under the nearest-neighbour model (not in the reference;
// catch_amd/filter/tm_filter.py defines the rule in integers and is its oracle), on the device's candidate list, before
// the near-duplicate filter and the set cover like the pre-filters of prefilter.hip.
//
// tm_flag_kernel: one thread per unique candidate, one pass over its L bytes, the rows staged as the poly(A) kernel
// stages them (stage.h).  Per byte one look-up of the dinucleotide (previous byte, this byte) in the 16-entry table of
// (|h|, |e|): it is indexed by data, so it lives in LDS, 16 dwords behind the staged rows, |h| in the low and |e| in the
// high half of a dword (at most 106 and 272) -- 16 consecutive dwords are 16 different banks, and lanes on one dword
// are served by a broadcast, so whatever dinucleotides the lanes of a wave hold the look-up has no bank conflict.  Only
// the table's entries are packed: the two sums are 64-bit registers each (|E| passes 65,535 at 300 bases, |H| at
// 1,000, and L is not bounded), the initiation terms and the signs are applied after the walk.  Then
//     E' = 100 E + q,   T = H < 0 ? 10^7 (-H) / (-E') : 0,   tm_c = T - offset_c
// with ONE unsigned 64-bit division per candidate; q <= -8200 keeps E' negative wherever H < 0 (the host checks it).
// Counting: behind the table, TM_WORDS 64-bit counters per workgroup -- the 128 bins of whole degrees, then "below" and
// "above".  The threads add their multiplicities to the bins with LDS atomics (exact u64 sums; Tm piles into about 15
// neighbouring bins, which are different banks, and adds to one bin queue in LDS for a few cycles, not in L2); "below"
// and "above" are two addresses for most of the threads of a filtering call, so they are summed over the wave first
// (wave_sum_n) and added once per wave (8.9 M candidates, a range that drops 2 in 3: 0.656 ms; 0.709 with every thread
// adding).  After a barrier thread t adds counter t, if it is not zero, to one of TM_SLOTS copies in global memory, which the host adds
// up: a wave's adds are neighbouring u64s of one or two 128-byte lines, and the copy is chosen by the workgroup's
// number, so that the 35,000 workgroups of 8.9 M candidates do not queue on the same 15 lines (prefilter.hip's
// COMP_SLOTS records what one copy costs).  A copy is TM_SLOT_WORDS = 144 words, 9 whole lines.  No thread returns
// before the barrier.  FILTER = false writes no flag and HIST = false touches no bin.
#include "internal.h"
#include "wave.h"
#include "stage.h"

#define TM_BINS 128u
#define TM_WORDS 130u                // the bins, below, above
#define TM_SLOTS 64u
#define TM_SLOT_WORDS 144u
#define TM_TABLE_DW 16u
#define TM_EXTRA_BYTES (TM_TABLE_DW * 4u + TM_WORDS * 8u)       // behind the rows: 1,104 bytes per workgroup

// |h| | |e| << 16 of the dinucleotide (first, second), index 4 * first + second with 'A' 0, 'C' 1, 'T' 2, 'G' 3
// ((c >> 1) & 3 of the byte): SantaLucia 1998, h in 100 cal/mol, e in 0.1 cal/(K mol)
#define TM_NN(h, e) ((u32)(h) | ((u32)(e) << 16))
__constant__ u32 tm_nn_table[TM_TABLE_DW] = {
    TM_NN(79, 222), TM_NN(84, 224), TM_NN(72, 204), TM_NN(78, 210),       // AA AC AT AG
    TM_NN(85, 227), TM_NN(80, 199), TM_NN(78, 210), TM_NN(106, 272),      // CA CC CT CG
    TM_NN(72, 213), TM_NN(82, 222), TM_NN(79, 222), TM_NN(85, 227),       // TA TC TT TG
    TM_NN(82, 222), TM_NN(98, 244), TM_NN(84, 224), TM_NN(80, 199)};      // GA GC GT GG

template <bool STAGE, bool FILTER, bool HIST>
__global__ void __launch_bounds__(256)
tm_flag_kernel(const u8 *__restrict__ bytes, const u32 *__restrict__ upos, const u32 *__restrict__ mult, u32 n, u32 L,
               i64 q, i64 offset_c, i64 lo_c, i64 hi_c, u32 nchunk, u32 pitch_dw, u32 extra_off_dw,
               u32 *__restrict__ flag, u64 *__restrict__ totals) {
    extern __shared__ u32 tm_lds[];
    const u32 rows = blockDim.x, r = threadIdx.x;
    const u32 i = blockIdx.x * rows + r;
    u32 *tbl = tm_lds + extra_off_dw;                                               // (extra_off_dw is even: 8-byte aligned)
    unsigned long long *cnt = (unsigned long long *)(tbl + TM_TABLE_DW);
    if (r < TM_TABLE_DW) tbl[r] = tm_nn_table[r];
    for (u32 t = r; t < TM_WORDS; t += rows) cnt[t] = 0;
    if (STAGE) stage_rows(bytes, upos, n, L, nchunk, pitch_dw, tm_lds);             // (ends with a barrier)
    else __syncthreads();
    u64 t_below = 0, t_above = 0;
    if (i < n) {                                              // (no early return: the wave sums and the barrier below)
        const u32 s = upos[i];
        const u8 *p = STAGE ? (const u8 *)(tm_lds + r * pitch_dw) + (s & 15u) : bytes + s;
        u64 sh = 0, se = 0;                                   // -sum of h, -sum of e over the dinucleotides
        u32 pc = 0;
        bool pb = false;
        for (u32 j = 0; j < L; ++j) {
            const u8 c = p[j];
            const bool b = is_base(c);
            const u32 code = (c >> 1) & 3u;
            const u32 v = (b && pb) ? tbl[(pc << 2) | code] : 0u;
            sh += v & 0xffffu;
            se += v >> 16;
            pc = code;
            pb = b;
        }
        const u8 c0 = p[0], c1 = p[L - 1];
        const bool g0 = c0 == 'G' || c0 == 'C', g1 = c1 == 'G' || c1 == 'C';
        const i64 H = (g0 ? 1 : 23) + (g1 ? 1 : 23) - (i64)sh;
        const i64 E = (g0 ? -28 : 41) + (g1 ? -28 : 41) - (i64)se;
        const i64 E1 = 100 * E + q;                           // < 0 wherever H < 0
        const i64 T = H < 0 ? (i64)((10000000ull * (u64)(-H)) / (u64)(-E1)) : 0;
        const i64 tm_c = T - offset_c;
        const u32 m = mult[i];
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
    if (FILTER) {
        wave_sum_n(t_below, t_above);
        if ((r & 63u) == 0) {
            if (t_below) atomicAdd(cnt + TM_BINS, (unsigned long long)t_below);
            if (t_above) atomicAdd(cnt + TM_BINS + 1u, (unsigned long long)t_above);
        }
    }
    __syncthreads();
    unsigned long long *t = (unsigned long long *)totals + (blockIdx.x & (TM_SLOTS - 1u)) * TM_SLOT_WORDS;
    for (u32 w = r; w < TM_WORDS; w += rows) {
        const unsigned long long v = cnt[w];
        if (v) atomicAdd(t + w, v);
    }
}

template <bool FILTER, bool HIST>
static int launch_tm(catchhip_ctx *ctx, const catchhip_candidates *C, i64 q, i64 offset_c, i64 lo_c, i64 hi_c, u32 *flag,
                     u64 *totals) {
    const u32 n = (u32)C->nuniq, L = (u32)C->L;
    // the rows as the poly(A) kernel stages them, and behind them the table and the counters, once per workgroup
    const u32 nchunk = (L + 15u + 15u) / 16u, pitch_dw = 4u * nchunk + 1u;
    const size_t row_bytes = (size_t)pitch_dw * 4;
    u32 rows = 256;
    while (rows > 64 && rows * row_bytes + TM_EXTRA_BYTES > POLYA_LDS_BUDGET) rows >>= 1;
    const bool stage = rows * row_bytes + TM_EXTRA_BYTES <= POLYA_LDS_BUDGET && ((uintptr_t)C->T->bytes.p & 15u) == 0;
    if (stage)
        hipLaunchKernelGGL((tm_flag_kernel<true, FILTER, HIST>), dim3((unsigned)div_up((i64)n, rows)), dim3(rows),
                           rows * row_bytes + TM_EXTRA_BYTES, ctx->stream, (const u8 *)C->T->bytes.p,
                           (const u32 *)C->upos.p, (const u32 *)C->mult.p, n, L, q, offset_c, lo_c, hi_c, nchunk, pitch_dw,
                           rows * pitch_dw, flag, totals);
    else
        hipLaunchKernelGGL((tm_flag_kernel<false, FILTER, HIST>), dim3((unsigned)div_up((i64)n, 256)), dim3(256),
                           TM_EXTRA_BYTES, ctx->stream, (const u8 *)C->T->bytes.p, (const u32 *)C->upos.p,
                           (const u32 *)C->mult.p, n, L, q, offset_c, lo_c, hi_c, nchunk, pitch_dw, 0u, flag, totals);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int catchhip_candidates_drop_tm(catchhip_ctx *ctx, catchhip_candidates *C, i64 q, i32 offset_c, i32 filter_on,
                                           i32 lo_c, i32 hi_c, i64 dropped[3], u64 hist[128], i64 *nkept) {
    ARG_CHECK(ctx && C && C->ctx == ctx);
    if (C->filtered) {
        chip_set_error("candidates_drop_tm: a near-duplicate filter was already applied (the Tm filter comes first)");
        return CATCHHIP_EINVAL;
    }
    if (q > -8200) {
        chip_set_error("candidates_drop_tm: q must be <= -8200, so that 100 E + q stays negative (got %lld)", (long long)q);
        return CATCHHIP_EINVAL;
    }
    if (filter_on && lo_c > hi_c) {
        chip_set_error("candidates_drop_tm: lo_c exceeds hi_c (got %d, %d)", (int)lo_c, (int)hi_c);
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    if (nkept) *nkept = C->nuniq;
    if (dropped) dropped[0] = dropped[1] = dropped[2] = 0;
    if (hist) memset(hist, 0, sizeof(u64) * TM_BINS);
    if (C->nuniq == 0 || C->L < 2 || !(filter_on || hist)) return 0;
    const u32 n = (u32)C->nuniq;
    DevBuf<u32> flag;
    DevBuf<u64> totals;
    if (filter_on) TRY(flag.alloc((size_t)n + 1));
    const size_t totals_bytes = sizeof(u64) * TM_SLOTS * TM_SLOT_WORDS;
    TRY(totals.alloc(TM_SLOTS * TM_SLOT_WORDS));
    TRY(chip_pinned_reserve(ctx, totals_bytes));
    HIP_TRY(hipMemsetAsync(totals.p, 0, totals_bytes, ctx->stream));
    PhaseTimer tm(ctx, PHASE_PREFILTER);
    if (filter_on && hist) TRY((launch_tm<true, true>(ctx, C, q, offset_c, lo_c, hi_c, flag.p, totals.p)));
    else if (filter_on) TRY((launch_tm<true, false>(ctx, C, q, offset_c, lo_c, hi_c, flag.p, totals.p)));
    else TRY((launch_tm<false, true>(ctx, C, q, offset_c, 0, 0, nullptr, totals.p)));
    tm.launch();
    tm.stop();
    HIP_TRY(hipMemcpyAsync(ctx->h_big, totals.p, totals_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    tm.finish();
    u64 below = 0, above = 0;
    for (u32 slot = 0; slot < TM_SLOTS; ++slot) {
        const u64 *w = (const u64 *)ctx->h_big + slot * TM_SLOT_WORDS;
        if (hist) for (u32 b = 0; b < TM_BINS; ++b) hist[b] += w[b];
        below += w[TM_BINS];
        above += w[TM_BINS + 1u];
    }
    if (dropped) { dropped[0] = (i64)below; dropped[1] = (i64)above; dropped[2] = (i64)(below + above); }
    if (below + above == 0) return 0;                         // nothing dropped (or not filtering): the list stands
    return chip_candidates_keep_flagged(ctx, C, flag, nkept);
}
