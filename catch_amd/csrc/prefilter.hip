// Filters that are a function of the candidate alone, on the device's candidate list -- they run before the
// near-duplicate filter and the set cover, where the reference runs them before the duplicate filter.
//
// PolyAFilter (catch/filter/polya_filter.py:43-71): a candidate is dropped iff
//   * it holds an exact run of >= min_exact 'A' or of >= min_exact 'T' (the reference's gate before its slow
//     call; it changes answers, so it is part of the rule; min_exact == 0 lets everything through), and
//   * for c = 'A' or c = 'T' its longest common substring with c * L under `mismatches` mismatches
//     (Probe.longest_common_substring_length, an O(L^2) k_lcf per candidate) is >= length.
// The second condition asks for a window of >= length characters of which at most `mismatches` differ from c.
// Every such window contains one of exactly `length` characters with no more mismatches, so "the longest window
// is >= length" is "some window of `length` characters has <= mismatches mismatches": two pointers `length`
// apart, one pass, the same two characters read for 'A' and for 'T'.  Any character but c is a mismatch ('N' too).
//
// polya_flag_kernel: one thread per unique candidate, O(L).  A candidate's characters sit in the targets' byte
// array at upos[i] and the candidates of a workgroup overlap (stride < length), so the workgroup first copies its
// rows into LDS -- 16-byte loads from the 16-byte boundary below each row's start, consecutive lanes on
// consecutive chunks of a row -- and both pointers of the walk read LDS.  The row pitch is an odd number of
// dwords: the lanes of a wave read the same column of 64 different rows, which an even pitch would put on a
// few banks.  Rows too long for 64 of them to fit the LDS budget are read from global memory (L is not bounded).
#include "internal.h"
#include "wave.h"
#include "stage.h"

template <bool STAGE>
__global__ void __launch_bounds__(256)
polya_flag_kernel(const u8 *__restrict__ bytes, const u32 *__restrict__ upos, u32 n, u32 L, u32 length, u32 k,
                  u32 min_exact, u32 nchunk, u32 pitch_dw, u32 *__restrict__ flag) {
    extern __shared__ u32 polya_lds[];
    const u32 rows = blockDim.x, r = threadIdx.x;
    const u32 base = blockIdx.x * rows;
    if (STAGE) stage_rows(bytes, upos, n, L, nchunk, pitch_dw, polya_lds);
    const u32 i = base + r;
    if (i >= n) return;
    const u32 s = upos[i];
    const u8 *p = STAGE ? (const u8 *)(polya_lds + r * pitch_dw) + (s & 15u) : bytes + s;
    u32 mm_a = 0, mm_t = 0, run_a = 0, run_t = 0, best_run = 0;
    bool hit = false;
    for (u32 j = 0; j < L; ++j) {
        const u8 c = p[j];
        const bool a = c == 'A', t = c == 'T';
        run_a = a ? run_a + 1 : 0;
        run_t = t ? run_t + 1 : 0;
        best_run = max(best_run, max(run_a, run_t));
        mm_a += a ? 0u : 1u;
        mm_t += t ? 0u : 1u;
        if (j >= length) {
            const u8 o = p[j - length];
            mm_a -= o == 'A' ? 0u : 1u;
            mm_t -= o == 'T' ? 0u : 1u;
        }
        if (j + 1 >= length) hit |= mm_a <= k || mm_t <= k;
    }
    flag[i] = (hit && best_run >= min_exact) ? 0u : 1u;       // (min_exact == 0: every candidate passes the gate)
}

extern "C" int catchhip_candidates_drop_polya(catchhip_ctx *ctx, catchhip_candidates *C, i32 length, i32 mismatches,
                                              i32 min_exact, i64 *nkept) {
    ARG_CHECK(ctx && C && C->ctx == ctx);
    if (C->filtered) {
        chip_set_error("candidates_drop_polya: a near-duplicate filter was already applied (the poly(A) filter comes first)");
        return CATCHHIP_EINVAL;
    }
    if (length < 1 || mismatches < 0 || min_exact < 0) {
        chip_set_error("candidates_drop_polya: length must be >= 1, mismatches and min_exact >= 0 (got %d, %d, %d)",
                       (int)length, (int)mismatches, (int)min_exact);
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    if (nkept) *nkept = C->nuniq;
    if (C->nuniq == 0 || length > C->L) return 0;             // a stretch longer than the candidates: nothing to drop
    const u32 n = (u32)C->nuniq, L = (u32)C->L;
    DevBuf<u32> flag;
    TRY(flag.alloc((size_t)n + 1));
    // a row in LDS: from the 16-byte boundary below its start (<= 15 bytes before it) to its end
    const u32 nchunk = (L + 15u + 15u) / 16u, pitch_dw = 4u * nchunk + 1u;
    u32 rows = 256;
    while (rows > 64 && (size_t)rows * pitch_dw * 4 > POLYA_LDS_BUDGET) rows >>= 1;
    const bool stage = (size_t)rows * pitch_dw * 4 <= POLYA_LDS_BUDGET && ((uintptr_t)C->T->bytes.p & 15u) == 0;
    PhaseTimer tm(ctx, PHASE_PREFILTER);
    if (stage)
        hipLaunchKernelGGL(polya_flag_kernel<true>, dim3((unsigned)div_up((i64)n, rows)), dim3(rows),
                           (size_t)rows * pitch_dw * 4, ctx->stream, (const u8 *)C->T->bytes.p, (const u32 *)C->upos.p, n,
                           L, (u32)length, (u32)mismatches, (u32)min_exact, nchunk, pitch_dw, flag.p);
    else
        hipLaunchKernelGGL(polya_flag_kernel<false>, dim3((unsigned)div_up((i64)n, 256)), dim3(256), 0, ctx->stream,
                           (const u8 *)C->T->bytes.p, (const u32 *)C->upos.p, n, L, (u32)length, (u32)mismatches,
                           (u32)min_exact, nchunk, pitch_dw, flag.p);
    HIP_TRY(hipGetLastError());
    tm.launch();
    tm.stop();
    TRY(chip_candidates_keep_flagged(ctx, C, flag, nkept));
    tm.finish();
    return 0;
}

// ---- composition rules (not in the reference; catch_amd/filter/composition_filter.py defines them) -------------------
// composition_flag_kernel: one thread per unique candidate, one pass over its L bytes, the rows staged as above.
//   GC and the homopolymer run are counters in registers.
//   Low complexity (DUST = true): the window's 64 triplet counters c_t are indexed by data, so they live in LDS, one
//   byte each (a window of <= 256 bytes holds <= 254 triplets).  Layout, behind the staged rows: dword g * rows + r
//   holds the counters of codes 4g .. 4g + 3 of thread r -- a lane's pitch is ONE dword and a code group's pitch is
//   `rows` dwords (a multiple of 32), so whatever codes the lanes of a wave touch, lane l is on bank l mod 32: the 32
//   lanes that a byte access serves per cycle never share a bank.  A thread touches its own counters only (no barrier).
//   The window moves one byte per step: the triplet that leaves (c_t--, S -= c_t), then the one that enters
//   (S += c_t, c_t++); a second pointer We - 2 bytes behind the first rebuilds the leaving triplet's code.
//   DUST = false allocates no counters and does no triplet work.
// The per-rule totals (with multiplicity) are summed over the wave, then one atomic per wave and non-zero counter --
// into one of COMP_SLOTS copies of the four totals, a 128-byte line each, which the host adds up: with one copy, the
// 140,000 waves of 8.9 M candidates queued on a single line and the atomics took longer than the walk.
#define COMP_COUNTER_BYTES 64u
#define COMP_SLOTS 64u
#define COMP_SLOT_WORDS 16u

template <bool STAGE, bool DUST>
__global__ void __launch_bounds__(256)
composition_flag_kernel(const u8 *__restrict__ bytes, const u32 *__restrict__ upos, const u32 *__restrict__ mult, u32 n,
                        u32 L, u32 gc_lo, u32 gc_hi, u32 max_run, u32 x10, u32 We, u32 nchunk, u32 pitch_dw,
                        u32 cnt_off_dw, u32 *__restrict__ flag, u64 *__restrict__ totals) {
    extern __shared__ u32 comp_lds[];
    const u32 rows = blockDim.x, r = threadIdx.x;
    const u32 i = blockIdx.x * rows + r;
    if (STAGE) stage_rows(bytes, upos, n, L, nchunk, pitch_dw, comp_lds);
    u32 fail = 0, m = 0;
    if (i < n) {                                              // (no early return: the wave sums below need every lane)
        const u32 s = upos[i];
        const u8 *p = STAGE ? (const u8 *)(comp_lds + r * pitch_dw) + (s & 15u) : bytes + s;
        u8 *cnt = (u8 *)(comp_lds + cnt_off_dw + r);          // counter of code t: cnt[(t >> 2) * 4 * rows + (t & 3)]
        if (DUST)
            for (u32 g = 0; g < COMP_COUNTER_BYTES / 4u; ++g) comp_lds[cnt_off_dw + g * rows + r] = 0;
        u32 gc = 0, run = 0, best_run = 0, prev = 0;
        u32 h = 0, v = 0, ho = 0, vo = 0, S = 0, T = 0;       // head and tail triplet (code, which of its bytes are bases)
        bool low = false;
        for (u32 j = 0; j < L; ++j) {
            const u8 c = p[j];
            const bool b = is_base(c);
            gc += (c == 'G' || c == 'C') ? 1u : 0u;
            run = b ? (c == prev ? run + 1 : 1u) : 0u;
            prev = c;
            best_run = max(best_run, run);
            if (DUST) {
                if (j + 2 >= We) {                            // triplet j - We leaves (its last byte is j + 2 - We < j)
                    const u8 o = p[j + 2 - We];
                    ho = ((ho << 2) | ((o >> 1) & 3u)) & 63u;
                    vo = ((vo << 1) | (is_base(o) ? 1u : 0u)) & 7u;
                    if (vo == 7u) {
                        u8 *q = cnt + (ho >> 2) * 4u * rows + (ho & 3u);
                        const u32 ct = *q - 1u;
                        *q = (u8)ct;
                        S -= ct;
                        --T;
                    }
                }
                h = ((h << 2) | ((c >> 1) & 3u)) & 63u;       // 'A' 0, 'C' 1, 'T' 2, 'G' 3: any numbering gives the same S
                v = ((v << 1) | (b ? 1u : 0u)) & 7u;
                if (v == 7u) {                                // triplet j - 2 enters
                    u8 *q = cnt + (h >> 2) * 4u * rows + (h & 3u);
                    const u32 ct = *q;
                    *q = (u8)(ct + 1u);
                    S += ct;
                    ++T;
                }
                if (j + 1 >= We) low |= T >= 2 && 10u * S > x10 * (T - 1u);     // a whole window: starts at j + 1 - We
            }
        }
        fail = ((gc < gc_lo || gc > gc_hi) ? 1u : 0u) | (best_run > max_run ? 2u : 0u) | (low ? 4u : 0u);
        flag[i] = fail ? 0u : 1u;
        m = mult[i];
    }
    u64 t_gc = (fail & 1u) ? m : 0u, t_run = (fail & 2u) ? m : 0u, t_low = (fail & 4u) ? m : 0u, t_any = fail ? m : 0u;
    wave_sum_n(t_gc, t_run, t_low, t_any);
    if ((r & 63u) == 0) {
        unsigned long long *t = (unsigned long long *)totals + (blockIdx.x & (COMP_SLOTS - 1u)) * COMP_SLOT_WORDS;
        if (t_gc) atomicAdd(t + 0, (unsigned long long)t_gc);
        if (t_run) atomicAdd(t + 1, (unsigned long long)t_run);
        if (t_low) atomicAdd(t + 2, (unsigned long long)t_low);
        if (t_any) atomicAdd(t + 3, (unsigned long long)t_any);
    }
}

template <bool DUST>
static int launch_composition(catchhip_ctx *ctx, const catchhip_candidates *C, u32 gc_lo, u32 gc_hi, u32 max_run, u32 x10,
                              u32 We, u32 *flag, u64 *totals) {
    const u32 n = (u32)C->nuniq, L = (u32)C->L;
    // the rows as the poly(A) kernel stages them, and behind them COMP_COUNTER_BYTES per row when the counters are there
    const u32 nchunk = (L + 15u + 15u) / 16u, pitch_dw = 4u * nchunk + 1u;
    const size_t row_bytes = (size_t)pitch_dw * 4, cnt_bytes = DUST ? COMP_COUNTER_BYTES : 0u;
    u32 rows = 256;
    while (rows > 64 && rows * (row_bytes + cnt_bytes) > POLYA_LDS_BUDGET) rows >>= 1;
    const bool stage = rows * (row_bytes + cnt_bytes) <= POLYA_LDS_BUDGET && ((uintptr_t)C->T->bytes.p & 15u) == 0;
    if (stage)
        hipLaunchKernelGGL((composition_flag_kernel<true, DUST>), dim3((unsigned)div_up((i64)n, rows)), dim3(rows),
                           rows * (row_bytes + cnt_bytes), ctx->stream, (const u8 *)C->T->bytes.p, (const u32 *)C->upos.p,
                           (const u32 *)C->mult.p, n, L, gc_lo, gc_hi, max_run, x10, We, nchunk, pitch_dw, rows * pitch_dw,
                           flag, totals);
    else
        hipLaunchKernelGGL((composition_flag_kernel<false, DUST>), dim3((unsigned)div_up((i64)n, 256)), dim3(256),
                           256 * cnt_bytes, ctx->stream, (const u8 *)C->T->bytes.p, (const u32 *)C->upos.p,
                           (const u32 *)C->mult.p, n, L, gc_lo, gc_hi, max_run, x10, We, nchunk, pitch_dw, 0u, flag,
                           totals);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int catchhip_candidates_drop_composition(catchhip_ctx *ctx, catchhip_candidates *C, i32 gc_lo, i32 gc_hi,
                                                    i32 max_run, i32 dust_x10, i32 dust_window, i64 dropped[4],
                                                    i64 *nkept) {
    ARG_CHECK(ctx && C && C->ctx == ctx);
    if (C->filtered) {
        chip_set_error("candidates_drop_composition: a near-duplicate filter was already applied (the composition filter comes first)");
        return CATCHHIP_EINVAL;
    }
    if (gc_lo < -1 || gc_hi < -1 || max_run < -1 || max_run == 0 || dust_x10 < -1 ||
        (dust_x10 >= 0 && (dust_window < 3 || dust_window > 256))) {
        chip_set_error("candidates_drop_composition: gc_lo, gc_hi >= 0, max_run >= 1, dust_x10 >= 0 (or -1: off) and "
                       "3 <= dust_window <= 256 (got %d, %d, %d, %d, %d)",
                       (int)gc_lo, (int)gc_hi, (int)max_run, (int)dust_x10, (int)dust_window);
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    if (nkept) *nkept = C->nuniq;
    if (dropped) dropped[0] = dropped[1] = dropped[2] = dropped[3] = 0;
    const bool gc_on = gc_lo > 0 || (gc_hi >= 0 && gc_hi < C->L);
    const bool dust_on = dust_x10 >= 0 && C->L >= 4;          // (a window of < 4 bytes holds < 2 triplets)
    if (C->nuniq == 0 || !(gc_on || max_run > 0 || dust_on)) return 0;
    const u32 n = (u32)C->nuniq;
    DevBuf<u32> flag;
    DevBuf<u64> totals;
    TRY(flag.alloc((size_t)n + 1));
    const size_t totals_bytes = sizeof(u64) * COMP_SLOTS * COMP_SLOT_WORDS;
    TRY(totals.alloc(COMP_SLOTS * COMP_SLOT_WORDS));
    TRY(chip_pinned_reserve(ctx, totals_bytes));
    HIP_TRY(hipMemsetAsync(totals.p, 0, totals_bytes, ctx->stream));
    PhaseTimer tm(ctx, PHASE_PREFILTER);
    const u32 lo = gc_lo < 0 ? 0u : (u32)gc_lo, hi = gc_hi < 0 ? 0xffffffffu : (u32)gc_hi;
    const u32 run = max_run < 0 ? 0xffffffffu : (u32)max_run;
    if (dust_on) {
        // 10 S <= 10 * 254 * 253 / 2 = 321,310: any larger threshold drops nothing, and x10 * (T - 1) stays in 32 bits
        const u32 x10 = (u32)(dust_x10 < 400000 ? dust_x10 : 400000);
        const u32 We = (u32)(dust_window < C->L ? dust_window : C->L);
        TRY(launch_composition<true>(ctx, C, lo, hi, run, x10, We, flag.p, totals.p));
    } else {
        TRY(launch_composition<false>(ctx, C, lo, hi, run, 0u, 0u, flag.p, totals.p));
    }
    tm.launch();
    tm.stop();
    HIP_TRY(hipMemcpyAsync(ctx->h_big, totals.p, totals_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    tm.finish();
    u64 h[4] = {0, 0, 0, 0};
    for (u32 slot = 0; slot < COMP_SLOTS; ++slot)
        for (int k = 0; k < 4; ++k) h[k] += ((const u64 *)ctx->h_big)[slot * COMP_SLOT_WORDS + k];
    if (dropped) for (int k = 0; k < 4; ++k) dropped[k] = (i64)h[k];
    if (h[3] == 0) return 0;                                  // nothing dropped: the list stands
    return chip_candidates_keep_flagged(ctx, C, flag, nkept);
}

// the multiplicities the filter must carry along (tests compare them; the near-duplicate filters read them on the device)
extern "C" int catchhip_candidates_multiplicities(catchhip_ctx *ctx, const catchhip_candidates *C, u32 *mult) {
    ARG_CHECK(ctx && C && C->ctx == ctx);
    if (C->filtered) {
        chip_set_error("candidates_multiplicities: not kept once a near-duplicate filter was applied");
        return CATCHHIP_EINVAL;
    }
    if (C->nuniq == 0) return 0;
    ARG_CHECK(mult);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(mult, C->mult.p, sizeof(u32) * (size_t)C->nuniq, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}
