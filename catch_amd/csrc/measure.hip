// The value behind every candidate rule instead of a verdict at one threshold (not in the reference;
// catch_amd/filter/quality.py defines the five integers gc, homopolymer, dust, stem, dimer and is their oracle; tm_c and
// hits are TmFilter._tm_c and BackgroundFilter._hits), on the device's candidate list, before the near-duplicate
// filter.  The list is only read.  Two kernels, because their LDS holds different things:
//
// measure_rows_kernel<STAGE, COMP, TM, HITS, M>: gc, homopolymer, dust, tm_c and hits -- one thread per unique candidate,
//   one pass over its L bytes, the rows staged (stage.h).  The per-byte work of each family is that of its flag kernel
//   (prefilter.hip, thermo.hip, background.hip): Tm and hits through the same steppers of stage.h and the look-ups of
//   kmer_lookup.h, exact or within the index's mismatches; gc, homopolymer and the window's step written out as in
//   composition_flag_kernel (prefilter.hip says why the two do not share a stepper).  What differs is the end:
//   dust.  The flag kernel compares every window with ONE threshold; the measure keeps the running maximum `best` of
//   ceil(10 S / (T - 1)) and asks the flag kernel's question with it, 10 S > best (T - 1), which is true iff the
//   window's quotient exceeds best.  Only then is the quotient formed: one integer division per RISE of the maximum,
//   not per window (10 S <= 321,310 and best (T - 1) <= 1,270 * 253: 32 bits).
//
// measure_structure_kernel<LDS_PLANES>: stem and dimer -- one thread per unique candidate, the L x L table pairs(x, y)
//   32 cells at a time, over the planes and the antidiagonal words of planes.h, as structure_flag_kernel walks them.
//   What differs:
//   Run search.  There is no R to look for: each lane keeps `best`, the longest run it has seen, per rule.  A run that
//   touches a word's edge is measured, not searched: carry + (1-cells that begin the word) and the 1-cells that end it
//   are lengths, and best takes their maximum.  A run strictly inside a word is found by the flag kernel's question for
//   best + 1 -- five AND-shifts whose amounts are per-lane registers (planes.h: RunShifts) -- and where the answer is yes the
//   survivors are AND-shifted one step at a time until none is left, which gives the word's longest run exactly.  best
//   settles on the first antidiagonals (a random 100-mer reaches 6 within a few words), so nearly every word costs the
//   question alone: 2 count-zeros, 5 shift-ANDs, 3 maxima and two branches not taken per rule; the shift amounts are
//   recomputed only when best rises (about 15 operations, a few times per candidate).
//   Range of c.  c = 1 .. 2 L - 3 (the antidiagonals 0 and 2 L - 2 are one cell (x, x), which never pairs), each walked
//   over x = lo .. floor(c / 2), lo = max(0, c - L + 1): HALF an antidiagonal.  Proof that nothing is missed:
//   pairs(x, y) = pairs(y, x), so cell x of antidiagonal c equals cell c - x.  A run [a, b] that lies at or below the
//   middle (b <= c / 2) is seen whole.  One above it is the mirror image of [c - b, c - a], which is seen.  One across
//   the middle exists only for odd c (for even c the middle cell pairs with itself: never a 1-cell); being maximal and
//   the table symmetric it is its own mirror image, [a, c - a], of c - 2 a + 1 cells, of which a .. (c - 1) / 2 are
//   seen: exactly half.  So for odd c the run that ENDS on the last walked cell counts twice its seen length, and this
//   is exact, not a bound.  The hairpin rule sees the same words cut at cell (c - 1 - P) / 2 <= (c - 1) / 2 and never
//   doubles: a stem's inner end is its run's last cell, so stem = the longest run among the cells x <= (c - 1 - P) / 2.
//   No antidiagonal is skipped for being shorter than best: best is per lane, the walk is per wave, and the ones that
//   short are one word each.
//   Work per candidate: the sum over c of (c / 2 >> 5) - (lo >> 5) + 1 words -- 302 words of 32 cells for L = 100
//   (the flag kernel walks 308 at D = 11, the whole table is 496), each 6 LDS reads, 3 funnel shifts, 4 logic
//   operations and the two searches above (about 45 operations).
//   Where the planes live: in LDS, or in a global buffer when 64 candidates' planes and the bins do not fit.
//
// Histograms (five, MEASURE_BINS bins each, bin min(value, MEASURE_BINS - 1), with multiplicity): per workgroup in
// LDS behind the rows or planes, as many 64-bit bins per quantity as its values can reach at this L and window, added
// to with LDS atomics; after a barrier the bins go to one of MEASURE_SLOTS copies in global memory (stage.h: the
// totals).  No thread returns before the barrier.  Without histograms no bin is allocated or touched.
#include "internal.h"
#include "wave.h"
#include "stage.h"
#include "planes.h"
#include "rule_host.h"
#include "kmer_lookup.h"

typedef uint16_t u16;

#define MEASURE_BINS 1280u
#define MEASURE_SLOTS 32u
#define MEASURE_SLOT_WORDS (5u * MEASURE_BINS)               // 400 whole 128-byte lines

struct MeasureRowsArgs {
    const u8 *bytes;                 // the row arguments field by field (row_args() below makes stage.h's RowArgs of them):
    const u32 *upos, *mult;          // with a RowArgs member the other fields moved, the kernel's scalar loads were cut
    u32 n, L, nchunk, pitch_dw;      // differently and the composition instances ran 1 % slower
    u32 We;                          // composition: the window, min(W, L); 0: no window holds two triplets (dust = 0)
    i64 q, offset_c;                 // Tm
    u32 K, rc_shift, dir_shift;      // hits
    u64 mask;
    const u64 *codes;
    const u32 *dir;
    u32 cnt_off_dw, tbl_off_dw, bin_off_dw;      // LDS: triplet counters, dinucleotide table, bins (even: 8-byte aligned)
    u32 nb_len, nb_dust;             // bins of gc and of homopolymer, bins of dust; 0: no histograms
    u16 *gc, *run, *dust;            // per-candidate values (each may be null)
    i32 *tm_c;
    u32 *hits;
    u64 *hist;                       // MEASURE_SLOTS copies of the five histograms
    KmerViews views;                 // hits against a tolerant index (mismatches > 0)
    __host__ __device__ RowArgs row_args() const { return RowArgs{bytes, upos, mult, n, L, nchunk, pitch_dw, cnt_off_dw}; }
};

// M: the mismatch budget of the index behind `hits` (0: the exact look-up; 1, 2: HITS is on)
template <bool STAGE, bool COMP, bool TM, bool HITS, int M = 0>
__global__ void __launch_bounds__(256)
measure_rows_kernel(const MeasureRowsArgs a) {
    extern __shared__ u32 mr_lds[];
    const u32 rows = blockDim.x, r = threadIdx.x;
    const u32 i = blockIdx.x * rows + r;
    const RowArgs ra = a.row_args();
    const u32 L = a.L;
    u32 *tbl = mr_lds + a.tbl_off_dw;
    unsigned long long *bins = (unsigned long long *)(mr_lds + a.bin_off_dw);
    const u32 nbins = COMP ? 2u * a.nb_len + a.nb_dust : 0u;
    if (TM) TmSums::load_table(tbl);
    for (u32 t = r; t < nbins; t += rows) bins[t] = 0;
    if (STAGE) stage_rows(ra, mr_lds);                        // (ends with a barrier)
    else __syncthreads();
    if (i < a.n) {                                            // (no early return: the barrier below)
        const u8 *p = row_ptr<STAGE>(ra, mr_lds, i);
        const u32 We = a.We;
        // gc, homopolymer and the window, written out as in composition_flag_kernel (prefilter.hip says why)
        u8 *cnt = (u8 *)(mr_lds + a.cnt_off_dw + r);   // counter of code t: cnt[(t >> 2) * 4 * rows + (t & 3)]
        if (COMP && We)
            for (u32 g = 0; g < TRIPLET_COUNTER_BYTES / 4u; ++g) mr_lds[a.cnt_off_dw + g * rows + r] = 0;
        u32 gc = 0, run = 0, best_run = 0, prev = 0;
        u32 h = 0, v = 0, ho = 0, vo = 0, S = 0, T = 0, dust = 0;
        TmSums sums;
        KmerRoll kmer;
        u32 hits = 0;
        for (u32 j = 0; j < L; ++j) {
            const u8 c = p[j];
            const bool b = is_base(c);
            const u32 code = base_code(c);
            if (COMP) {
                gc += (c == 'G' || c == 'C') ? 1u : 0u;
                run = b ? (c == prev ? run + 1 : 1u) : 0u;
                prev = c;
                best_run = max(best_run, run);
                if (We) {
                    if (j + 2 >= We) {                        // triplet j - We leaves (its last byte is j + 2 - We < j)
                        const u8 o = p[j + 2 - We];
                        ho = ((ho << 2) | ((o >> 1) & 3u)) & 63u;
                        vo = ((vo << 1) | (is_base(o) ? 1u : 0u)) & 7u;
                        if (vo == 7u) {
                            u8 *cq = cnt + (ho >> 2) * 4u * rows + (ho & 3u);
                            const u32 ct = *cq - 1u;
                            *cq = (u8)ct;
                            S -= ct;
                            --T;
                        }
                    }
                    h = ((h << 2) | code) & 63u;
                    v = ((v << 1) | (b ? 1u : 0u)) & 7u;
                    if (v == 7u) {                            // triplet j - 2 enters
                        u8 *cq = cnt + (h >> 2) * 4u * rows + (h & 3u);
                        const u32 ct = *cq;
                        *cq = (u8)(ct + 1u);
                        S += ct;
                        ++T;
                    }
                    // a whole window (it starts at j + 1 - We) whose quotient exceeds the maximum so far
                    if (j + 1 >= We && T >= 2 && 10u * S > dust * (T - 1u)) dust = (10u * S + T - 2u) / (T - 1u);
                }
            }
            if (TM) sums.step(tbl, code, b);
            if (HITS && kmer.step(code, b, a.mask, a.rc_shift, a.K)) {
                if constexpr (M == 0) hits += kmer_lookup_exact(kmer.fwd, kmer.rc, a.codes, a.dir, a.dir_shift);
                else hits += kmer_lookup_tolerant<M>(kmer.fwd, kmer.rc, a.mask, 2u * a.K, a.views);
            }
        }
        if (COMP) {
            if (a.gc) a.gc[i] = (u16)gc;                    // (L <= 65,535: the host checked)
            if (a.run) a.run[i] = (u16)best_run;
            if (a.dust) a.dust[i] = (u16)dust;
            if (nbins) {
                const unsigned long long m = a.mult[i];
                atomicAdd(bins + min(gc, a.nb_len - 1u), m);
                atomicAdd(bins + a.nb_len + min(best_run, a.nb_len - 1u), m);
                atomicAdd(bins + 2u * a.nb_len + min(dust, a.nb_dust - 1u), m);
            }
        }
        if (TM && a.tm_c) {
            const i64 tm = sums.tm_c(p[0], p[L - 1], a.q, a.offset_c);
            a.tm_c[i] = tm > 2147483647ll ? 2147483647 : tm < -2147483647ll ? -2147483647 : (i32)tm;   // (E' near 0)
        }
        if (HITS && a.hits) a.hits[i] = hits;
    }
    if (nbins) {
        __syncthreads();
        // bin t of the workgroup: gc 0 .. nb_len - 1, homopolymer, dust.  The bins' last one stands for every value
        // from there up, which is MEASURE_BINS - 1 whenever a value can pass it (nb = MEASURE_BINS then)
        totals_flush(bins, nbins, totals_slot(a.hist, MEASURE_SLOTS, MEASURE_SLOT_WORDS), [&](u32 t) {
            const u32 qn = t < a.nb_len ? 0u : t < 2u * a.nb_len ? 1u : 2u;
            return qn * MEASURE_BINS + (t - qn * a.nb_len);
        });
    }
}

// The longest run of 1-bits in a stream of words, per lane.  best: the longest seen so far; shifts: the question "does
// a word hold best + 1 consecutive 1-bits".
struct RunMax {
    u32 best = 0;
    RunShifts shifts;
    __device__ __forceinline__ void aim() { shifts.aim(best + 1u); }
    // one word m of the stream: `low` 1-bits begin it, carry_in 1-bits ended the words before it, carry_out end the
    // words up to and including it (0 where the stream is cut inside this word)
    __device__ __forceinline__ void see(u32 m, u32 low, u32 carry_in, u32 carry_out) {
        u32 x = shifts.inside(m);                             // bit b of x <=> bits b .. b + best of m
        u32 b = max(best, max(carry_in + low, carry_out)), inside = best;
        while (x) { ++inside; x &= x >> 1; }                  // (rare) the word's longest run, one more cell per step
        b = max(b, inside);
        if (b != best) { best = b; aim(); }
    }
};

template <bool LDS_PLANES>
__global__ void __launch_bounds__(256)
measure_structure_kernel(const u8 *__restrict__ bytes, const u32 *__restrict__ upos, const u32 *__restrict__ mult, u32 first,
                         u32 n, u32 L, u32 W, u32 P, u32 *__restrict__ gplanes, u32 bin_off_dw, u32 nb,
                         u16 *__restrict__ stem_out, u16 *__restrict__ dimer_out, u64 *__restrict__ hist) {
    extern __shared__ u32 ms_lds[];
    const u32 r = threadIdx.x;
    const u32 i = first + blockIdx.x * blockDim.x + r;
    u32 *pl = (LDS_PLANES ? ms_lds + r * plane_pitch(W) : gplanes + (size_t)(blockIdx.x * blockDim.x + r) * plane_pitch(W));
    unsigned long long *bins = (unsigned long long *)(ms_lds + bin_off_dw);         // stem 0 .. nb - 1, then dimer
    for (u32 t = r; t < 2u * nb; t += blockDim.x) bins[t] = 0;
    if (nb) __syncthreads();
    if (i < n) {                                              // (no early return: the barrier below)
        build_planes(bytes + upos[i], L, W, pl);
        RunMax rd, rh;
        rd.aim();
        rh.aim();
        for (u32 c = 1; c + 3u <= 2u * L; ++c) {              // c = 1 .. 2 L - 3 (none for L = 1)
            const u32 upto = c >> 1;                          // lo <= upto <= min(L - 1, c)
            const bool hair_here = c >= 1u + P;
            const u32 inner = hair_here ? (c - 1u - P) >> 1 : 0u;                   // the hairpin's last cell (<= upto)
            u32 carry = 0, carry_in = 0, m_last = 0;
            antidiagonal_words(pl, W, c, antidiagonal_lo(c, L), upto, [&](u32 w, u32 m) {
                const u32 inv = ~m;
                const u32 low = inv ? (u32)__builtin_ctz(inv) : 32u, high = inv ? (u32)__builtin_clz(inv) : 32u;
                carry_in = carry;
                carry = inv ? high : carry + 32u;
                rd.see(m, low, carry_in, carry);
                if (hair_here && 32u * w <= inner) {          // (the same in every lane)
                    const u32 last = inner - 32u * w;         // the word's last cell of the rule
                    if (last >= 31u) {
                        rh.see(m, low, carry_in, carry);
                    } else {
                        const u32 mh = m & ((2u << last) - 1u);                     // (bit 31 is 0: ~mh is not)
                        rh.see(mh, (u32)__builtin_ctz(~mh), carry_in, 0u);
                    }
                }
                m_last = m;
            });
            if (c & 1u) {
                // the run that ends on the last walked cell, bit `last` of the last word, is half of a run across the
                // middle: the 1-bits below and at `last`, and the carry when they fill the word from bit 0
                const u32 last = upto & 31u;
                const u32 zeros = ~m_last & (last >= 31u ? 0xffffffffu : (2u << last) - 1u);
                const u32 seen = zeros ? last + (u32)__builtin_clz(zeros) - 31u : carry_in + last + 1u;
                if (2u * seen > rd.best) { rd.best = 2u * seen; rd.aim(); }
            }
        }
        if (stem_out) stem_out[i] = (u16)rh.best;             // (<= L <= 65,535: the host checked)
        if (dimer_out) dimer_out[i] = (u16)rd.best;
        if (nb) {
            const unsigned long long mi = mult[i];
            atomicAdd(bins + min(rh.best, nb - 1u), mi);
            atomicAdd(bins + nb + min(rd.best, nb - 1u), mi);
        }
    }
    if (nb) {
        __syncthreads();
        totals_flush(bins, 2u * nb, totals_slot(hist, MEASURE_SLOTS, MEASURE_SLOT_WORDS), [&](u32 t) {
            const u32 qn = t < nb ? 0u : 1u;
            return (3u + qn) * MEASURE_BINS + (t - qn * nb);
        });
    }
}

// ---- the launches --------------------------------------------------------------------------------------------------
typedef void (*measure_rows_fn)(const MeasureRowsArgs);
template <bool STAGE>
static measure_rows_fn measure_rows_instance(bool comp, bool tm, bool hits) {
    static const measure_rows_fn table[8] = {
        nullptr,
        measure_rows_kernel<STAGE, true, false, false>, measure_rows_kernel<STAGE, false, true, false>,
        measure_rows_kernel<STAGE, true, true, false>, measure_rows_kernel<STAGE, false, false, true>,
        measure_rows_kernel<STAGE, true, false, true>, measure_rows_kernel<STAGE, false, true, true>,
        measure_rows_kernel<STAGE, true, true, true>};
    return table[(comp ? 1 : 0) | (tm ? 2 : 0) | (hits ? 4 : 0)];
}
template <bool STAGE, int M>
static measure_rows_fn measure_rows_tolerant_instance(bool comp, bool tm) {
    static const measure_rows_fn table[4] = {
        measure_rows_kernel<STAGE, false, false, true, M>, measure_rows_kernel<STAGE, true, false, true, M>,
        measure_rows_kernel<STAGE, false, true, true, M>, measure_rows_kernel<STAGE, true, true, true, M>};
    return table[(comp ? 1 : 0) | (tm ? 2 : 0)];
}

static int launch_measure_rows(catchhip_ctx *ctx, const catchhip_candidates *C, bool comp, bool tm, bool hits,
                               i32 mismatches, bool histograms, MeasureRowsArgs a) {
    const u32 L = (u32)C->L;
    a.nb_len = comp && histograms ? std::min(L, MEASURE_BINS - 1u) + 1u : 0u;
    a.nb_dust = comp && histograms ? (a.We ? std::min(5u * (a.We - 2u), MEASURE_BINS - 1u) + 1u : 1u) : 0u;
    // LDS: the rows, then per row the triplet counters, then once per workgroup the dinucleotide table and the bins
    const size_t tbl_bytes = tm ? TM_TABLE_DW * 4u : 0u, bin_bytes = (size_t)(2u * a.nb_len + a.nb_dust) * 8;
    const RowPlan plan = row_plan(L, comp && a.We ? TRIPLET_COUNTER_BYTES : 0u, tbl_bytes + bin_bytes, 8, rows_aligned(C));
    const RowArgs ra = row_args(C, plan);
    a.bytes = ra.bytes; a.upos = ra.upos; a.mult = ra.mult;
    a.n = ra.n; a.L = ra.L; a.nchunk = ra.nchunk; a.pitch_dw = ra.pitch_dw;
    a.cnt_off_dw = ra.extra_off_dw;
    a.tbl_off_dw = plan.tail_off_dw;
    a.bin_off_dw = plan.tail_off_dw + (u32)(tbl_bytes / 4);   // (even: the table is 16 dwords)
    const bool stage = plan.stage;
    measure_rows_fn fn = stage ? measure_rows_instance<true>(comp, tm, hits) : measure_rows_instance<false>(comp, tm, hits);
    if (hits && mismatches == 1)
        fn = stage ? measure_rows_tolerant_instance<true, 1>(comp, tm) : measure_rows_tolerant_instance<false, 1>(comp, tm);
    if (hits && mismatches == 2)
        fn = stage ? measure_rows_tolerant_instance<true, 2>(comp, tm) : measure_rows_tolerant_instance<false, 2>(comp, tm);
    hipLaunchKernelGGL(fn, row_grid(C, plan), dim3(plan.rows), plan.lds_bytes, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int launch_measure_structure(catchhip_ctx *ctx, const catchhip_candidates *C, u32 P, bool histograms, u16 *stem,
                                    u16 *dimer, u64 *hist) {
    const u32 n = (u32)C->nuniq, L = (u32)C->L;
    const u32 nb = histograms ? std::min(L, MEASURE_BINS - 1u) + 1u : 0u;
    const PlanePlan plan = plane_plan(L, (size_t)2 * nb * 8, 8);
    const u8 *bytes = (const u8 *)C->T->bytes.p;
    const u32 *upos = (const u32 *)C->upos.p, *mult = (const u32 *)C->mult.p;
    if (plan.lds_planes) {
        hipLaunchKernelGGL((measure_structure_kernel<true>), dim3((unsigned)div_up((i64)n, plan.rows)), dim3(plan.rows),
                           plan.lds_bytes, ctx->stream, bytes, upos, mult, 0u, n, L, plan.W, P, (u32 *)nullptr,
                           plan.tail_off_dw, nb, stem, dimer, hist);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    return launch_over_plane_chunks(ctx, n, plan.cand_bytes, [&](u32 first, u32 end, u32 *planes) {
        hipLaunchKernelGGL((measure_structure_kernel<false>), dim3((unsigned)div_up((i64)(end - first), 256)), dim3(256),
                           plan.lds_bytes, ctx->stream, bytes, upos, mult, first, end, L, plan.W, P, planes, 0u, nb, stem,
                           dimer, hist);
    });
}

template <typename T>
static int measure_fetch(catchhip_ctx *ctx, const DevBuf<T> &d, T *out, size_t n) {
    if (out) HIP_TRY(hipMemcpyAsync(out, d.p, sizeof(T) * n, hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

extern "C" int catchhip_candidates_measure(catchhip_ctx *ctx, const catchhip_candidates *C, u32 what, i32 min_loop,
                                           i32 dust_window, i64 q, i32 offset_c, const catchhip_kmer_index *X,
                                           i32 want_values, u16 *gc, u16 *homopolymer, u16 *dust, u16 *stem, u16 *dimer,
                                           i32 *tm_c, u32 *hits, u64 *hist) {
    ARG_CHECK(ctx && C && C->ctx == ctx);
    TRY(rule_refuse_filtered(C, "candidates_measure", "measure"));
    const bool comp = what & CATCHHIP_MEASURE_COMPOSITION, structure = what & CATCHHIP_MEASURE_STRUCTURE;
    const bool tm = what & CATCHHIP_MEASURE_TM, bg = what & CATCHHIP_MEASURE_HITS;
    if (what & ~15u) {
        chip_set_error("candidates_measure: what is a mask of the bits 1 (composition), 2 (structure), 4 (Tm) and 8 "
                       "(hits) (got %u)", (unsigned)what);
        return CATCHHIP_EINVAL;
    }
    if ((comp && (dust_window < 3 || dust_window > 256)) || (structure && min_loop < 0)) {
        chip_set_error("candidates_measure: 3 <= dust_window <= 256 and min_loop >= 0 (got %d, %d)", (int)dust_window,
                       (int)min_loop);
        return CATCHHIP_EINVAL;
    }
    if (tm && q > -8200) {
        chip_set_error("candidates_measure: q must be <= -8200, so that 100 E + q stays negative (got %lld)", (long long)q);
        return CATCHHIP_EINVAL;
    }
    if (bg && !X) {
        chip_set_error("candidates_measure: hits need an index");
        return CATCHHIP_EINVAL;
    }
    if (bg && X->device != ctx->device) {
        chip_set_error("candidates_measure: the index lives on device %d, the candidates on device %d", X->device,
                       ctx->device);
        return CATCHHIP_EINVAL;
    }
    if (what && C->L > 65535) {
        chip_set_error("candidates_measure: candidates of more than 65,535 characters are not measured (got %d)", (int)C->L);
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    TRY(rule_begin(ctx, C, nullptr));
    if (hist) memset(hist, 0, sizeof(u64) * MEASURE_SLOT_WORDS);
    if (C->nuniq == 0 || !what || !(want_values || hist)) return 0;
    const size_t n = (size_t)C->nuniq;
    const u32 L = (u32)C->L;
    if (want_values) {
        ARG_CHECK(!comp || (gc && homopolymer && dust));
        ARG_CHECK(!structure || (stem && dimer));
        ARG_CHECK(!tm || tm_c);
        ARG_CHECK(!bg || hits);
    }
    const bool tm_on = tm && want_values && L >= 2;           // (Tm and hits have no histogram here: values or nothing)
    const bool bg_on = bg && want_values && (i64)L >= X->k;
    if (tm && want_values && !tm_on)
        for (size_t i = 0; i < n; ++i) tm_c[i] = CATCHHIP_MEASURE_NO_TM;
    if (bg && want_values && !bg_on) memset(hits, 0, sizeof(u32) * n);
    DevBuf<u16> d_gc, d_run, d_dust, d_stem, d_dimer;
    DevBuf<i32> d_tm;
    DevBuf<u32> d_hits;
    SlotTotals d_hist;
    if (hist && (comp || structure)) TRY(d_hist.init(ctx, MEASURE_SLOTS, MEASURE_SLOT_WORDS));
    if (want_values && comp) { TRY(d_gc.alloc(n)); TRY(d_run.alloc(n)); TRY(d_dust.alloc(n)); }
    if (want_values && structure) { TRY(d_stem.alloc(n)); TRY(d_dimer.alloc(n)); }
    if (tm_on) TRY(d_tm.alloc(n));
    if (bg_on) TRY(d_hits.alloc(n));
    PhaseTimer timer(ctx, PHASE_PREFILTER);
    if (comp || tm_on || bg_on) {
        MeasureRowsArgs a = {};
        a.We = L >= 4 ? std::min((u32)dust_window, L) : 0u;   // (a window of < 4 bytes holds < 2 triplets)
        a.q = q;
        a.offset_c = offset_c;
        if (bg_on) {
            a.K = (u32)X->k;
            a.mask = a.K == 32 ? ~0ull : (((u64)1 << (2 * a.K)) - 1);
            a.rc_shift = 2 * a.K - 2;
            a.dir_shift = 2 * a.K - X->P;
            a.codes = X->codes;
            a.dir = X->dir;
            a.views = kmer_views(X);
        }
        a.gc = d_gc.p; a.run = d_run.p; a.dust = d_dust.p; a.tm_c = d_tm.p; a.hits = d_hits.p;
        a.hist = d_hist.d.p;
        TRY(launch_measure_rows(ctx, C, comp, tm_on, bg_on, bg_on ? X->mismatches : 0, hist != nullptr, a));
        timer.launch();
    }
    if (structure) {
        ARG_CHECK(((uintptr_t)C->T->bytes.p & 3u) == 0);      // (the kernel reads the candidates as aligned dwords)
        TRY(launch_measure_structure(ctx, C, (u32)min_loop, hist != nullptr, d_stem.p, d_dimer.p, d_hist.d.p));
        timer.launch();
    }
    timer.stop();
    if (want_values) {
        if (comp) { TRY(measure_fetch(ctx, d_gc, gc, n)); TRY(measure_fetch(ctx, d_run, homopolymer, n)); TRY(measure_fetch(ctx, d_dust, dust, n)); }
        if (structure) { TRY(measure_fetch(ctx, d_stem, stem, n)); TRY(measure_fetch(ctx, d_dimer, dimer, n)); }
        if (tm_on) TRY(measure_fetch(ctx, d_tm, tm_c, n));
        if (bg_on) TRY(measure_fetch(ctx, d_hits, hits, n));
    }
    if (d_hist.d.p) TRY(d_hist.read(ctx, MEASURE_SLOT_WORDS, hist));         // (synchronises: the values are there too)
    else HIP_TRY(hipStreamSynchronize(ctx->stream));
    timer.finish();
    return 0;
}
