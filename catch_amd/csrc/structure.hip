// Secondary-structure rules on the device's candidate list (not in the reference; catch_amd/filter/structure_filter.py
// defines them and is their oracle): a hairpin stem of more than K base pairs around a loop of at least P characters,
// a self-dimer of more than D consecutive base pairs.  Both ask for a run of R consecutive cells on an antidiagonal
// x + y = c of the candidate's L x L table pairs(x, y) -- R = D + 1 anywhere on it for the self-dimer; R = K + 1 among
// the cells x <= (c - 1 - P) / 2 for the hairpin (x the left arm: its inner end i + K and the right arm's inner end
// c - (i + K) then have P characters between them).
//
// structure_flag_kernel<HAIRPIN, DIMER, LDS_PLANES>: one thread per unique candidate, the table 32 cells at a time
// (planes.h: the bit planes, where they live, the word of an antidiagonal).
//   Runs.  A run of R cells is looked for word by word: inside the word by AND-shifts that double the run in hand
//   (planes.h: RunShifts; only for R <= 32), and across words by a counter of the 1-cells that end the previous word
//   (carry + the 1-cells that begin this word >= R).  The hairpin rule sees the same words cut at its last cell.
//   Every lane of a wave walks the same c and w: there is no divergence but the final flag.
//   Work per candidate: pairs(x, y) = pairs(y, x), so each antidiagonal is walked to just past its middle (shown
//   where the bound is formed): the sum over the antidiagonals c that can hold a run of (upto >> 5) - (lo >> 5) + 1
//   words, lo = max(0, c - L + 1), upto = min(L - 1, c, (c + D) / 2) -- 308 words of 32 cells for L = 100, D = 11 (the
//   table has 10,000 cells; walked whole it would be 496 words), each 6 LDS reads (4 instructions), 3 funnel shifts, 4
//   logic operations and the run search of each rule that is on (about 20 operations, no branch).
// The per-rule totals (with multiplicity) are summed over the wave, then one atomic per wave and non-zero counter into
// one of STRUCT_SLOTS padded copies (stage.h: the totals).
#include "internal.h"
#include "wave.h"
#include "stage.h"
#include "planes.h"
#include "rule_host.h"

#define STRUCT_SLOTS 64u
#define STRUCT_SLOT_WORDS 16u

// does the stream of words m (one call per word, ascending) hold R consecutive 1-bits?  carry: the 1-bits that end the
// words so far (0 before the first word); rs: aimed at R.
__device__ __forceinline__ bool run_step(u32 m, u32 &carry, u32 R, const RunShifts &rs) {
    const u32 inv = ~m;
    const u32 low_ones = inv ? (u32)__builtin_ctz(inv) : 32u, high_ones = inv ? (u32)__builtin_clz(inv) : 32u;
    const bool hit = carry + low_ones >= R || rs.inside(m) != 0;      // across words: the run that ends the words before goes on
    carry = inv ? high_ones : carry + 32u;
    return hit;
}

template <bool HAIRPIN, bool DIMER, bool LDS_PLANES>
__global__ void __launch_bounds__(256)
structure_flag_kernel(const u8 *__restrict__ bytes, const u32 *__restrict__ upos, const u32 *__restrict__ mult, u32 first,
                      u32 n, u32 L, u32 W, u32 K, u32 P, u32 D, u32 *__restrict__ gplanes, u32 *__restrict__ flag,
                      u64 *__restrict__ totals) {
    extern __shared__ u32 struct_lds[];
    const u32 r = threadIdx.x;
    const u32 i = first + blockIdx.x * blockDim.x + r;
    u32 *pl = (LDS_PLANES ? struct_lds + r * plane_pitch(W) : gplanes + (size_t)(blockIdx.x * blockDim.x + r) * plane_pitch(W));
    u32 fail = 0, m_i = 0;
    if (i < n) {                                              // (no early return: the wave sums below need every lane)
        build_planes(bytes + upos[i], L, W, pl);
        // ---- the antidiagonals that can hold the shortest run asked for
        const u32 Rh = K + 1u, Rd = D + 1u;
        RunShifts rs_h, rs_d;
        rs_h.aim(Rh);
        rs_d.aim(Rd);
        const u32 need = HAIRPIN && DIMER ? min(Rh, Rd) : HAIRPIN ? Rh : Rd;        // <= L (the host checked)
        bool hair = false, dimer = false;
        for (u32 c = need - 1u; c <= 2u * (L - 1u) - (need - 1u); ++c) {
            const u32 hi = min(L - 1u, c);
            // the hairpin's last cell: x <= (c - 1 - P) / 2
            const bool hair_here = HAIRPIN && c >= 1u + P;
            const u32 inner = hair_here ? (c - 1u - P) >> 1 : 0u;
            if (!DIMER && !hair_here) continue;
            // Half an antidiagonal is enough.  pairs is symmetric, so cell x equals cell c - x: a run that lies above
            // the middle has its mirror image below it, and a run across the middle (c odd; for even c the middle cell
            // pairs with itself: never) joins its mirror image into a symmetric run [a, c - a] of >= R cells, of which
            // the cells a .. a + R - 1 <= (c + R - 1) / 2 are seen.  The hairpin rule ends below the middle anyway.
            const u32 upto = min(hi, DIMER ? (c + Rd - 1u) >> 1 : inner);           // (lo <= upto wherever a run fits)
            u32 carry_d = 0, carry_h = 0;
            antidiagonal_words(pl, W, c, antidiagonal_lo(c, L), upto, [&](u32 w, u32 m) {
                if (DIMER) dimer |= run_step(m, carry_d, Rd, rs_d);
                if (HAIRPIN && hair_here && 32u * w <= inner) {
                    const u32 last = inner - 32u * w;         // the word's last cell of the rule
                    const u32 mh = last >= 31u ? m : m & ((2u << last) - 1u);
                    hair |= run_step(mh, carry_h, Rh, rs_h);
                }
            });
        }
        fail = (hair ? 1u : 0u) | (dimer ? 2u : 0u);
        flag[i] = fail ? 0u : 1u;
        m_i = mult[i];
    }
    const u64 t_hair = (fail & 1u) ? m_i : 0u, t_dimer = (fail & 2u) ? m_i : 0u, t_any = fail ? m_i : 0u;
    totals_add_per_wave(totals_slot(totals, STRUCT_SLOTS, STRUCT_SLOT_WORDS), t_hair, t_dimer, t_any);
}

typedef void (*structure_fn)(const u8 *, const u32 *, const u32 *, u32, u32, u32, u32, u32, u32, u32, u32 *, u32 *, u64 *);
static structure_fn structure_instance(bool hairpin, bool dimer, bool lds_planes) {      // (hairpin || dimer)
    static const structure_fn table[2][3] = {
        {structure_flag_kernel<true, false, false>, structure_flag_kernel<false, true, false>, structure_flag_kernel<true, true, false>},
        {structure_flag_kernel<true, false, true>, structure_flag_kernel<false, true, true>, structure_flag_kernel<true, true, true>}};
    return table[lds_planes ? 1 : 0][(hairpin ? 1 : 0) + (dimer ? 2 : 0) - 1];
}

extern "C" int catchhip_candidates_drop_structure(catchhip_ctx *ctx, catchhip_candidates *C, i32 max_stem, i32 min_loop,
                                                  i32 max_dimer, i64 dropped[3], i64 *nkept) {
    ARG_CHECK(ctx && C && C->ctx == ctx);
    TRY(rule_refuse_filtered(C, "candidates_drop_structure", "structure filter"));
    if (max_stem < -1 || max_stem == 0 || max_dimer < -1 || max_dimer == 0 || (max_stem >= 1 && min_loop < 0)) {
        chip_set_error("candidates_drop_structure: max_stem >= 1, max_dimer >= 1 (or -1: off) and min_loop >= 0 "
                       "(got %d, %d, %d)", (int)max_stem, (int)min_loop, (int)max_dimer);
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    TRY(rule_begin(ctx, C, nkept));
    if (dropped) dropped[0] = dropped[1] = dropped[2] = 0;
    // a rule whose shortest structure is longer than the candidates drops nothing
    const bool hair_on = max_stem >= 1 && (i64)C->L >= 2 * (i64)max_stem + 2 + (i64)min_loop;
    const bool dimer_on = max_dimer >= 1 && (i64)C->L >= (i64)max_dimer + 1;
    if (C->nuniq == 0 || !(hair_on || dimer_on)) return 0;
    ARG_CHECK(((uintptr_t)C->T->bytes.p & 3u) == 0);          // (the kernel reads the candidates as aligned dwords)
    const u32 n = (u32)C->nuniq, L = (u32)C->L;
    DevBuf<u32> flag;
    SlotTotals totals;
    TRY(flag.alloc((size_t)n + 1));
    TRY(totals.init(ctx, STRUCT_SLOTS, STRUCT_SLOT_WORDS));
    PhaseTimer tm(ctx, PHASE_PREFILTER);
    const u32 K = hair_on ? (u32)max_stem : 0u, P = hair_on ? (u32)min_loop : 0u, D = dimer_on ? (u32)max_dimer : 0u;
    const PlanePlan plan = plane_plan(L, 0, 4);
    const structure_fn kernel = structure_instance(hair_on, dimer_on, plan.lds_planes);
    const u8 *bytes = (const u8 *)C->T->bytes.p;
    const u32 *upos = (const u32 *)C->upos.p, *mult = (const u32 *)C->mult.p;
    if (plan.lds_planes) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)div_up((i64)n, plan.rows)), dim3(plan.rows), plan.lds_bytes, ctx->stream,
                           bytes, upos, mult, 0u, n, L, plan.W, K, P, D, (u32 *)nullptr, flag.p, totals.d.p);
        HIP_TRY(hipGetLastError());
    } else {
        TRY(launch_over_plane_chunks(ctx, n, plan.cand_bytes, [&](u32 first, u32 end, u32 *planes) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)div_up((i64)(end - first), 256)), dim3(256), plan.lds_bytes, ctx->stream,
                               bytes, upos, mult, first, end, L, plan.W, K, P, D, planes, flag.p, totals.d.p);
        }));
    }
    tm.launch();
    tm.stop();
    u64 h[3];
    TRY(totals.read(ctx, 3, h));
    tm.finish();
    if (dropped) for (int k = 0; k < 3; ++k) dropped[k] = (i64)h[k];
    return rule_keep(ctx, C, h[2] != 0, flag, nkept);
}
