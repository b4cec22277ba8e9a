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
// polya_flag_kernel: one thread per unique candidate, O(L), both pointers of the walk on the staged row (stage.h).
#include "internal.h"
#include "wave.h"
#include "stage.h"
#include "rule_host.h"

template <bool STAGE>
__global__ void __launch_bounds__(256)
polya_flag_kernel(const RowArgs a, u32 length, u32 k, u32 min_exact, u32 *__restrict__ flag) {
    extern __shared__ u32 polya_lds[];
    if (STAGE) stage_rows(a, polya_lds);
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const u8 *p = row_ptr<STAGE>(a, polya_lds, i);
    u32 mm_a = 0, mm_t = 0, run_a = 0, run_t = 0, best_run = 0;
    bool hit = false;
    for (u32 j = 0; j < a.L; ++j) {
        const u8 c = p[j];
        const bool isa = c == 'A', ist = c == 'T';
        run_a = isa ? run_a + 1 : 0;
        run_t = ist ? run_t + 1 : 0;
        best_run = max(best_run, max(run_a, run_t));
        mm_a += isa ? 0u : 1u;
        mm_t += ist ? 0u : 1u;
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
    TRY(rule_refuse_filtered(C, "candidates_drop_polya", "poly(A) filter"));
    if (length < 1 || mismatches < 0 || min_exact < 0) {
        chip_set_error("candidates_drop_polya: length must be >= 1, mismatches and min_exact >= 0 (got %d, %d, %d)",
                       (int)length, (int)mismatches, (int)min_exact);
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    TRY(rule_begin(ctx, C, nkept));
    if (C->nuniq == 0 || length > C->L) return 0;             // a stretch longer than the candidates: nothing to drop
    DevBuf<u32> flag;
    TRY(flag.alloc((size_t)C->nuniq + 1));
    const RowPlan plan = row_plan((u32)C->L, 0, 0, 4, rows_aligned(C));
    PhaseTimer tm(ctx, PHASE_PREFILTER);
    hipLaunchKernelGGL(plan.stage ? polya_flag_kernel<true> : polya_flag_kernel<false>, row_grid(C, plan), dim3(plan.rows),
                       plan.lds_bytes, ctx->stream, row_args(C, plan), (u32)length, (u32)mismatches, (u32)min_exact, flag.p);
    HIP_TRY(hipGetLastError());
    tm.launch();
    tm.stop();
    TRY(chip_candidates_keep_flagged(ctx, C, flag, nkept));
    tm.finish();
    return 0;
}

// ---- composition rules (not in the reference; catch_amd/filter/composition_filter.py defines them) -------------------
// composition_flag_kernel: one thread per unique candidate, one pass over its L bytes, the rows staged (stage.h).
//   GC and the homopolymer run are counters in registers.
//   Low complexity (DUST = true): the window's 64 triplet counters in LDS behind the staged rows (stage.h has their
//   layout, TRIPLET_COUNTER_BYTES per thread).  The window moves one byte per step: the triplet that leaves
//   (c_t--, S -= c_t), then the one that enters (S += c_t, c_t++); a second pointer We - 2 bytes behind the first
//   rebuilds the leaving triplet's code.  Every whole window is asked 10 S > x10 (T - 1).  DUST = false allocates no
//   counters and does no triplet work.
//   The per-byte step is written out here and again in measure_rows_kernel (measure.hip), which ends it differently:
//   as steppers shared by the two (state in a struct, the step a member) both kernels compiled to the same
//   instructions in another order and ran 0.8 % and 2 % slower, so each keeps its own text.  A
//   change to the step is made in both; tests/test_quality_measure.py compares the two kernels.
//   The arguments come one by one, the thresholds between the row arguments, and RowArgs is made inside: with the
//   struct as the argument the thresholds' scalar load sank below the walk, the loop then waited for all four of its
//   LDS reads at once, and the GC-only instances ran 0.6 % slower.
// The per-rule totals (with multiplicity) are summed over the wave, then one atomic per wave and non-zero counter --
// into one of COMP_SLOTS copies of the four totals, a 128-byte line each (stage.h: the totals).
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
    const RowArgs a = {bytes, upos, mult, n, L, nchunk, pitch_dw, cnt_off_dw};
    if (STAGE) stage_rows(a, comp_lds);
    u32 fail = 0, m = 0;
    if (i < n) {                                              // (no early return: the wave sums below need every lane)
        const u8 *p = row_ptr<STAGE>(a, comp_lds, i);
        u8 *cnt = (u8 *)(comp_lds + cnt_off_dw + r);          // counter of code t: cnt[(t >> 2) * 4 * rows + (t & 3)]
        if (DUST)
            for (u32 g = 0; g < TRIPLET_COUNTER_BYTES / 4u; ++g) comp_lds[cnt_off_dw + g * rows + r] = 0;
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
    const u64 t_gc = (fail & 1u) ? m : 0u, t_run = (fail & 2u) ? m : 0u, t_low = (fail & 4u) ? m : 0u, t_any = fail ? m : 0u;
    totals_add_per_wave(totals_slot(totals, COMP_SLOTS, COMP_SLOT_WORDS), t_gc, t_run, t_low, t_any);
}

typedef decltype(&composition_flag_kernel<false, false>) composition_fn;
static composition_fn composition_instance(bool stage, bool dust) {
    static const composition_fn table[4] = {composition_flag_kernel<false, false>, composition_flag_kernel<true, false>,
                                            composition_flag_kernel<false, true>, composition_flag_kernel<true, true>};
    return table[(stage ? 1 : 0) | (dust ? 2 : 0)];
}

extern "C" int catchhip_candidates_drop_composition(catchhip_ctx *ctx, catchhip_candidates *C, i32 gc_lo, i32 gc_hi,
                                                    i32 max_run, i32 dust_x10, i32 dust_window, i64 dropped[4],
                                                    i64 *nkept) {
    ARG_CHECK(ctx && C && C->ctx == ctx);
    TRY(rule_refuse_filtered(C, "candidates_drop_composition", "composition filter"));
    if (gc_lo < -1 || gc_hi < -1 || max_run < -1 || max_run == 0 || dust_x10 < -1 ||
        (dust_x10 >= 0 && (dust_window < 3 || dust_window > 256))) {
        chip_set_error("candidates_drop_composition: gc_lo, gc_hi >= 0, max_run >= 1, dust_x10 >= 0 (or -1: off) and "
                       "3 <= dust_window <= 256 (got %d, %d, %d, %d, %d)",
                       (int)gc_lo, (int)gc_hi, (int)max_run, (int)dust_x10, (int)dust_window);
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    TRY(rule_begin(ctx, C, nkept));
    if (dropped) dropped[0] = dropped[1] = dropped[2] = dropped[3] = 0;
    const bool gc_on = gc_lo > 0 || (gc_hi >= 0 && gc_hi < C->L);
    const bool dust_on = dust_x10 >= 0 && C->L >= 4;          // (a window of < 4 bytes holds < 2 triplets)
    if (C->nuniq == 0 || !(gc_on || max_run > 0 || dust_on)) return 0;
    DevBuf<u32> flag;
    SlotTotals totals;
    TRY(flag.alloc((size_t)C->nuniq + 1));
    TRY(totals.init(ctx, COMP_SLOTS, COMP_SLOT_WORDS));
    PhaseTimer tm(ctx, PHASE_PREFILTER);
    const u32 lo = gc_lo < 0 ? 0u : (u32)gc_lo, hi = gc_hi < 0 ? 0xffffffffu : (u32)gc_hi;
    const u32 run = max_run < 0 ? 0xffffffffu : (u32)max_run;
    // 10 S <= 10 * 254 * 253 / 2 = 321,310: any larger threshold drops nothing, and x10 * (T - 1) stays in 32 bits
    const u32 x10 = dust_on ? (u32)(dust_x10 < 400000 ? dust_x10 : 400000) : 0u;
    const u32 We = dust_on ? (u32)(dust_window < C->L ? dust_window : C->L) : 0u;
    const RowPlan plan = row_plan((u32)C->L, dust_on ? TRIPLET_COUNTER_BYTES : 0u, 0, 4, rows_aligned(C));
    // (the order is the kernel's: n, L, then gc_lo, gc_hi, max_run, x10, We, then nchunk, pitch_dw, the counters' offset --
    // thirteen u32 in a row, which the compiler cannot tell apart)
    const RowArgs a = row_args(C, plan);
    hipLaunchKernelGGL(composition_instance(plan.stage, dust_on), row_grid(C, plan), dim3(plan.rows), plan.lds_bytes,
                       ctx->stream, a.bytes, a.upos, a.mult, a.n, a.L, lo, hi, run, x10, We, a.nchunk, a.pitch_dw,
                       a.extra_off_dw, flag.p, totals.d.p);
    HIP_TRY(hipGetLastError());
    tm.launch();
    tm.stop();
    u64 h[4];
    TRY(totals.read(ctx, 4, h));
    tm.finish();
    if (dropped) for (int k = 0; k < 4; ++k) dropped[k] = (i64)h[k];
    return rule_keep(ctx, C, h[3] != 0, flag, nkept);
}

// the launch plans of rule_host.h as the entry points of the five files get them (tests/test_candidate_launch_plan.py)
extern "C" int catchhip_selftest_candidate_plan(i32 L, i64 row_extra, i64 wg_extra, i32 tail_align, i32 aligned16,
                                                i64 plane_tail, i32 plane_align, u32 *row_out, u32 *plane_out) {
    ARG_CHECK(L >= 1 && row_extra >= 0 && row_extra % 4 == 0 && wg_extra >= 0 && plane_tail >= 0 && row_out && plane_out);
    ARG_CHECK((tail_align == 4 || tail_align == 8) && (plane_align == 4 || plane_align == 8));
    const RowPlan r = row_plan((u32)L, (size_t)row_extra, (size_t)wg_extra, (u32)tail_align, aligned16 != 0);
    const u32 rows[7] = {r.rows, r.stage ? 1u : 0u, r.nchunk, r.pitch_dw, r.extra_off_dw, r.tail_off_dw, (u32)r.lds_bytes};
    memcpy(row_out, rows, sizeof(rows));
    const PlanePlan p = plane_plan((u32)L, (size_t)plane_tail, (u32)plane_align);
    const u32 planes[5] = {p.W, p.rows, p.lds_planes ? 1u : 0u, p.tail_off_dw, (u32)p.lds_bytes};
    memcpy(plane_out, planes, sizeof(planes));
    return 0;
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
