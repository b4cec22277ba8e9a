// Secondary-structure rules on the device's candidate list (not in the reference; catch_amd/filter/structure_filter.py
// defines them and is their oracle): a hairpin stem of more than K base pairs around a loop of at least P characters,
// a self-dimer of more than D consecutive base pairs.  Both ask for a run of R consecutive cells on an antidiagonal
// x + y = c of the candidate's L x L table pairs(x, y) -- R = D + 1 anywhere on it for the self-dimer; R = K + 1 among
// the cells x <= (c - 1 - P) / 2 for the hairpin (x the left arm: its inner end i + K and the right arm's inner end
// c - (i + K) then have P characters between them).
//
// structure_flag_kernel<HAIRPIN, DIMER, LDS_PLANES>: one thread per unique candidate, the table 32 cells at a time.
//   Bit planes.  The candidate becomes three planes of W = ceil(L / 32) words, bit x of a plane for character x: V (a
//   base), B0 and B1 (bits 1 and 2 of the byte: A 00, C 01, T 10, G 11 as B1 B0, so that a base and its complement
//   differ in B1 and agree in B0).  Each plane is stored a second time bit-reversed over the 32 W bits, between two
//   zero words: cell (x, c - x) needs bit c - x of a plane, which is bit x + (32 W - 1 - c) of the reversed one -- a
//   SHIFT of the reversed plane, the same for every x of the antidiagonal.  Word w of the antidiagonal is then
//       m = (B1[w] ^ rB1) & ~(B0[w] ^ rB0) & V[w] & rV,    r* = 32 bits of the reversed plane from bit 32 w + shift,
//   one funnel shift per plane over two neighbouring words, of which the lower one is the previous word's upper one.
//   Cells outside the table come out 0 by themselves: x >= L has V = 0, y >= L has rV = 0, y < 0 reads the zero word
//   behind the reversed plane and y >= 32 W the one in front of it (word indices -1 .. W, shown where they are formed).
//   Runs.  A run of R cells is looked for word by word: inside the word by AND-shifts that double the run in hand
//   (m & m >> 1 has a bit where two cells follow each other, ...; only for R <= 32), and across words by a counter of
//   the 1-cells that end the previous word (carry + the 1-cells that begin this word >= R).  The hairpin rule sees the
//   same words cut at its last cell.
//   Where the planes live.  They are indexed by the loop counters w and c, the same in every lane but not constants:
//   in LDS (LDS_PLANES), or in a global buffer when 64 candidates' planes do not fit the LDS budget (L > 1,312).  No
//   array is indexed in registers.  A thread's words are contiguous, at a pitch of 6 W + 7 words -- odd, so that the
//   lanes of a wave, which read the same word of 64 candidates, are on different banks -- and the three planes are
//   interleaved (word 3 w + p of plane p; the reversed ones, W + 2 words each, behind them): an iteration's six reads
//   are constant offsets from two pointers that advance by three words.  Every lane of a wave walks the same c and w:
//   there is no divergence but the final flag.
//   Work per candidate: pairs(x, y) = pairs(y, x), so each antidiagonal is walked to just past its middle (shown
//   where the bound is formed): the sum over the antidiagonals c that can hold a run of (upto >> 5) - (lo >> 5) + 1
//   words, lo = max(0, c - L + 1), upto = min(L - 1, c, (c + D) / 2) -- 308 words of 32 cells for L = 100, D = 11 (the
//   table has 10,000 cells; walked whole it would be 496 words), each 6 LDS reads (4 instructions), 3 funnel shifts, 4
//   logic operations and the run search of each rule that is on (about 20 operations, no branch).
// The per-rule totals (with multiplicity) go the way the composition kernel's do: summed over the wave, then one atomic
// per wave and non-zero counter into one of STRUCT_SLOTS padded copies, which the host adds up.
#include "internal.h"
#include "wave.h"

#define STRUCT_LDS_BUDGET 65536u
#define STRUCT_SLOTS 64u
#define STRUCT_SLOT_WORDS 16u
#define STRUCT_GLOBAL_PLANE_BYTES ((size_t)256 << 20)     // plane buffer of one launch when the planes are in global memory

// A run length R as the search uses it: the five shifts whose AND-shifts grow the run in hand 1 -> R inside a word (a
// shift of 0 leaves the word as it is: R reached), and a mask that is 0 when no word can hold the run (R > 32).
struct RunSearch {
    u32 R, inword, s0, s1, s2, s3, s4;
    __device__ __forceinline__ explicit RunSearch(u32 run) : R(run), inword(run <= 32u ? 0xffffffffu : 0u) {
        u32 have = 1, s[5];
        for (int k = 0; k < 5; ++k) {                         // (unrolled: s[] stays in registers) steps 1, 2, 4, 8, 16 at most
            s[k] = have < run ? min(have, run - have) & 31u : 0u;
            have += s[k];
        }
        s0 = s[0]; s1 = s[1]; s2 = s[2]; s3 = s[3]; s4 = s[4];
    }
};

// does the stream of words m (one call per word, ascending) hold R consecutive 1-bits?  carry: the 1-bits that end the
// words so far (0 before the first word).
__device__ __forceinline__ bool run_step(u32 m, u32 &carry, const RunSearch &rs) {
    const u32 inv = ~m;
    const u32 low_ones = inv ? (u32)__builtin_ctz(inv) : 32u, high_ones = inv ? (u32)__builtin_clz(inv) : 32u;
    u32 x = m & rs.inword;                                    // a run inside the word: bit b of x <=> bits b .. b + have - 1 of m
    x &= x >> rs.s0;
    x &= x >> rs.s1;
    x &= x >> rs.s2;
    x &= x >> rs.s3;
    x &= x >> rs.s4;
    const bool hit = carry + low_ones >= rs.R || x != 0;      // or across words: the run that ends the words before goes on
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
    // this thread's 6 W + 6 words: word w of V, B0, B1 at pl[3 w + 0, 1, 2]; word q of the reversed planes (a zero word,
    // the plane, a zero word: q = 0 .. W + 1) at rev[3 q + 0, 1, 2]
    const u32 pitch = 6u * W + 7u;
    u32 *pl = (LDS_PLANES ? struct_lds + r * pitch : gplanes + (size_t)(blockIdx.x * blockDim.x + r) * pitch);
    u32 *rev = pl + 3u * W;
    u32 fail = 0, m_i = 0;
    if (i < n) {                                              // (no early return: the wave sums below need every lane)
        // ---- the planes, from the candidate's bytes read as aligned dwords (at most 3 bytes before the row, which
        // are the targets' own, and 3 behind it, inside the slack of the byte array)
        const u8 *row = bytes + upos[i];
        const u32 al = (u32)((uintptr_t)row & 3u);
        const u32 *dw = (const u32 *)(row - al);
        for (u32 p = 0; p < 3u; ++p) { rev[p] = 0; rev[3u * (W + 1u) + p] = 0; }
        u32 cur = dw[0], nd = 1;                              // cur: the dword that holds byte j
        for (u32 w = 0; w < W; ++w) {
            u32 v = 0, b0 = 0, b1 = 0;
            const u32 cnt = min(32u, L - 32u * w);
            for (u32 t = 0; t < cnt; ++t) {
                const u32 at = al + 32u * w + t;              // byte offset from dw
                if (at != 0 && (at & 3u) == 0) cur = dw[nd++];                  // nd - 1 = at / 4 <= (al + L - 1) / 4
                const u32 c = (cur >> (8u * (at & 3u))) & 255u;
                const u32 base = (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? 1u : 0u;
                v |= base << t;
                b0 |= ((c >> 1) & 1u) << t;
                b1 |= ((c >> 2) & 1u) << t;
            }
            pl[3u * w] = v;
            pl[3u * w + 1u] = b0;
            pl[3u * w + 2u] = b1;
            // bit z of a reversed plane = bit 32 W - 1 - z of the plane: word W - 1 - w, bits reversed; + 1: the zero word
            rev[3u * (W - w)] = __brev(v);
            rev[3u * (W - w) + 1u] = __brev(b0);
            rev[3u * (W - w) + 2u] = __brev(b1);
        }
        // ---- the antidiagonals that can hold the shortest run asked for
        const RunSearch rs_h(K + 1u), rs_d(D + 1u);
        const u32 need = HAIRPIN && DIMER ? min(rs_h.R, rs_d.R) : HAIRPIN ? rs_h.R : rs_d.R;    // <= L (the host checked)
        bool hair = false, dimer = false;
        for (u32 c = need - 1u; c <= 2u * (L - 1u) - (need - 1u); ++c) {
            const u32 lo = c > L - 1u ? c - (L - 1u) : 0u, hi = min(L - 1u, c);
            // cell (x, c - x) reads bit 32 W - 1 - c + x of a reversed plane, which is bit x + sh of the stored one (a
            // zero word in front: + 32), sh = 32 W + 31 - c.  sh may be "negative" (c up to 64 W - 2): it is kept mod
            // 2^32, and 32 w0 + sh is a true bit index again -- 32 w0 >= lo - 31 >= c - L - 30 gives 32 w0 + sh >=
            // 32 W - L + 1 >= 1, and 32 w1 <= hi <= c gives 32 w1 + sh <= 32 W + 31: stored words 0 .. W, and W + 1
            // as the upper word of the last funnel shift.  32 w does not touch the low five bits: one o for all w.
            const u32 sh = 32u * W + 31u - c;
            const u32 o = sh & 31u;
            // the hairpin's last cell: x <= (c - 1 - P) / 2
            const bool hair_here = HAIRPIN && c >= 1u + P;
            const u32 inner = hair_here ? (c - 1u - P) >> 1 : 0u;
            if (!DIMER && !hair_here) continue;
            // Half an antidiagonal is enough.  pairs is symmetric, so cell x equals cell c - x: a run that lies above
            // the middle has its mirror image below it, and a run across the middle (c odd; for even c the middle cell
            // pairs with itself: never) joins its mirror image into a symmetric run [a, c - a] of >= R cells, of which
            // the cells a .. a + R - 1 <= (c + R - 1) / 2 are seen.  The hairpin rule ends below the middle anyway.
            const u32 upto = min(hi, DIMER ? (c + rs_d.R - 1u) >> 1 : inner);
            const u32 w0 = lo >> 5, w1 = upto >> 5;             // (lo <= upto wherever a run fits; else w1 < w0: no words)
            const u32 *pf = pl + 3u * w0, *pr = rev + 3u * ((32u * w0 + sh) >> 5);
            u32 lv = pr[0], l0 = pr[1], l1 = pr[2];
            u32 carry_d = 0, carry_h = 0;
            for (u32 w = w0; w <= w1; ++w, pf += 3, pr += 3) {
                const u32 hv = pr[3], h0 = pr[4], h1 = pr[5];                   // reversed word q + 1 <= W + 1
                const u32 rv = __funnelshift_r(lv, hv, o), r0 = __funnelshift_r(l0, h0, o), r1 = __funnelshift_r(l1, h1, o);
                lv = hv; l0 = h0; l1 = h1;
                const u32 m = (pf[2] ^ r1) & ~(pf[1] ^ r0) & pf[0] & rv;
                if (DIMER) dimer |= run_step(m, carry_d, rs_d);
                if (HAIRPIN && hair_here && 32u * w <= inner) {
                    const u32 last = inner - 32u * w;         // the word's last cell of the rule
                    const u32 mh = last >= 31u ? m : m & ((2u << last) - 1u);
                    hair |= run_step(mh, carry_h, rs_h);
                }
            }
        }
        fail = (hair ? 1u : 0u) | (dimer ? 2u : 0u);
        flag[i] = fail ? 0u : 1u;
        m_i = mult[i];
    }
    u64 t_hair = (fail & 1u) ? m_i : 0u, t_dimer = (fail & 2u) ? m_i : 0u, t_any = fail ? m_i : 0u;
    wave_sum_n(t_hair, t_dimer, t_any);
    if ((r & 63u) == 0) {
        unsigned long long *t = (unsigned long long *)totals + (blockIdx.x & (STRUCT_SLOTS - 1u)) * STRUCT_SLOT_WORDS;
        if (t_hair) atomicAdd(t + 0, (unsigned long long)t_hair);
        if (t_dimer) atomicAdd(t + 1, (unsigned long long)t_dimer);
        if (t_any) atomicAdd(t + 2, (unsigned long long)t_any);
    }
}

template <bool HAIRPIN, bool DIMER>
static int launch_structure(catchhip_ctx *ctx, const catchhip_candidates *C, u32 K, u32 P, u32 D, u32 *flag, u64 *totals) {
    const u32 n = (u32)C->nuniq, L = (u32)C->L, W = (L + 31u) / 32u;
    const size_t cand_bytes = (size_t)(6u * W + 7u) * 4;      // three planes, three reversed ones between zero words, odd pitch
    const u8 *bytes = (const u8 *)C->T->bytes.p;
    u32 rows = 256;
    while (rows > 64 && rows * cand_bytes > STRUCT_LDS_BUDGET) rows >>= 1;
    if (rows * cand_bytes <= STRUCT_LDS_BUDGET) {
        hipLaunchKernelGGL((structure_flag_kernel<HAIRPIN, DIMER, true>), dim3((unsigned)div_up((i64)n, rows)), dim3(rows),
                           rows * cand_bytes, ctx->stream, bytes, (const u32 *)C->upos.p, (const u32 *)C->mult.p, 0u, n, L,
                           W, K, P, D, (u32 *)nullptr, flag, totals);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // planes in global memory, as many candidates per launch as the buffer holds (a multiple of the workgroup);
    // CATCHHIP_STRUCT_PLANE_BYTES, a test hook, shrinks the buffer so that a small list takes several launches
    const size_t budget = (size_t)chip_test_env_int("CATCHHIP_STRUCT_PLANE_BYTES", (long long)STRUCT_GLOBAL_PLANE_BYTES);
    u32 per = (u32)std::min<size_t>(budget / cand_bytes, (size_t)n);
    per = std::max(256u, (per + 255u) & ~255u);
    DevBuf<u32> planes;
    TRY(planes.alloc((size_t)per * (cand_bytes / 4)));
    for (u32 first = 0; first < n; first += per) {
        const u32 end = (u32)std::min<u64>((u64)first + per, n);
        hipLaunchKernelGGL((structure_flag_kernel<HAIRPIN, DIMER, false>), dim3((unsigned)div_up((i64)(end - first), 256)),
                           dim3(256), 0, ctx->stream, bytes, (const u32 *)C->upos.p, (const u32 *)C->mult.p, first, end, L,
                           W, K, P, D, planes.p, flag, totals);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));               // (the plane buffer goes back to the pool on return)
    return 0;
}

extern "C" int catchhip_candidates_drop_structure(catchhip_ctx *ctx, catchhip_candidates *C, i32 max_stem, i32 min_loop,
                                                  i32 max_dimer, i64 dropped[3], i64 *nkept) {
    ARG_CHECK(ctx && C && C->ctx == ctx);
    if (C->filtered) {
        chip_set_error("candidates_drop_structure: a near-duplicate filter was already applied (the structure filter comes first)");
        return CATCHHIP_EINVAL;
    }
    if (max_stem < -1 || max_stem == 0 || max_dimer < -1 || max_dimer == 0 || (max_stem >= 1 && min_loop < 0)) {
        chip_set_error("candidates_drop_structure: max_stem >= 1, max_dimer >= 1 (or -1: off) and min_loop >= 0 "
                       "(got %d, %d, %d)", (int)max_stem, (int)min_loop, (int)max_dimer);
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    if (nkept) *nkept = C->nuniq;
    if (dropped) dropped[0] = dropped[1] = dropped[2] = 0;
    // a rule whose shortest structure is longer than the candidates drops nothing
    const bool hair_on = max_stem >= 1 && (i64)C->L >= 2 * (i64)max_stem + 2 + (i64)min_loop;
    const bool dimer_on = max_dimer >= 1 && (i64)C->L >= (i64)max_dimer + 1;
    if (C->nuniq == 0 || !(hair_on || dimer_on)) return 0;
    ARG_CHECK(((uintptr_t)C->T->bytes.p & 3u) == 0);          // (the kernel reads the candidates as aligned dwords)
    const u32 n = (u32)C->nuniq;
    DevBuf<u32> flag;
    DevBuf<u64> totals;
    TRY(flag.alloc((size_t)n + 1));
    const size_t totals_bytes = sizeof(u64) * STRUCT_SLOTS * STRUCT_SLOT_WORDS;
    TRY(totals.alloc(STRUCT_SLOTS * STRUCT_SLOT_WORDS));
    TRY(chip_pinned_reserve(ctx, totals_bytes));
    HIP_TRY(hipMemsetAsync(totals.p, 0, totals_bytes, ctx->stream));
    PhaseTimer tm(ctx, PHASE_PREFILTER);
    const u32 K = hair_on ? (u32)max_stem : 0u, P = hair_on ? (u32)min_loop : 0u, D = dimer_on ? (u32)max_dimer : 0u;
    if (hair_on && dimer_on) TRY((launch_structure<true, true>(ctx, C, K, P, D, flag.p, totals.p)));
    else if (hair_on) TRY((launch_structure<true, false>(ctx, C, K, P, D, flag.p, totals.p)));
    else TRY((launch_structure<false, true>(ctx, C, K, P, D, flag.p, totals.p)));
    tm.launch();
    tm.stop();
    HIP_TRY(hipMemcpyAsync(ctx->h_big, totals.p, totals_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    tm.finish();
    u64 h[3] = {0, 0, 0};
    for (u32 slot = 0; slot < STRUCT_SLOTS; ++slot)
        for (int k = 0; k < 3; ++k) h[k] += ((const u64 *)ctx->h_big)[slot * STRUCT_SLOT_WORDS + k];
    if (dropped) for (int k = 0; k < 3; ++k) dropped[k] = (i64)h[k];
    if (h[2] == 0) return 0;                                  // nothing dropped: the list stands
    return chip_candidates_keep_flagged(ctx, C, flag, nkept);
}
