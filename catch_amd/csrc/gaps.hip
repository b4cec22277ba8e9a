// Uncovered regions of a row table (catchhip_rows_uncovered): where a probe set does not reach.  A region is a
// maximal run of bases at depth < min_depth inside one universe (one universe per sequence); it is reported when it
// has min_length bases and min_unambig of them are A, C, G or T.
//
//   1. chip_depth_array, chip_depth_bitmap (depth.hip)  depth per base, exact in 32 bits, and cov = the bitmap of
//                           the bases at depth >= min_depth; the depth array is handed back to the pool here
//   2. gp_boundary_kernel   bnd = the bitmap of the first bases of the non-empty universes (a lane per universe,
//                           atomicOr: commutes)
//      gp_acgt_kernel       with targets: acgt = the bitmap of the bases that are A, C, G or T (a lane per base,
//                           one __ballot per 64-bit word)
//      gp_mask_kernel       catchhip_rows_uncovered_within only: cov |= the mask's unwanted bases (a lane per word), so
//                           that a base nobody wants ends a run as a covered base does
//   3. gp_count_kernel      a lane per word: U = the uncovered bits; a run starts at an uncovered base whose
//                           predecessor is covered or which is a universe's first (bnd), and ends at one whose
//                           successor is covered or a universe's first -- shifts, one carry bit from each neighbour
//                           word, and bnd.  Popcounts of the start and the end marks per word.
//   4. chip_exclusive_scan_u32 twice: the number of starts / ends before every word.  The i-th start and the i-th
//                           end belong to region i, so
//   5. gp_emit_kernel       (a lane per word, the marks computed again) writes rs[] and re[] in position order:
//                           no sort, no atomics
//   6. gp_measure_kernel    a lane per region: length, and the popcount of acgt over it.  Regions of up to GP_SHORT
//                           words are counted by their lane; the longer ones of a wavefront are taken one after the
//                           other by the whole wavefront, 64 words per step.  flag = passes both filters
//   7. chip_exclusive_scan_u32 of the flags
//   8. gp_compact_kernel    a lane per region: the reported ones go to their place in the output table, with their
//                           universe (find_segment) and their unambiguous count in the set_id column; regions,
//                           bases and longest per universe by atomicAdd / atomicMax on 64-bit integers (a wavefront
//                           whose regions all lie in one universe reduces first)
//
// Everything is integer arithmetic and every atomic commutes: the result depends neither on the launch geometry nor on
// the order of the atomics.  Two counts come back to the host on the way (regions, reported regions): they size the
// arrays.  Scratch: 4 (total + 2) bytes of depth, given back before step 3; three bitmaps of total / 8 bytes (cov,
// bnd, acgt); 8 bytes per 64 bases of counts; 20 bytes per region before the filters (rs, re, unambiguous count,
// flag, place); the output table has 16 bytes per reported region.
#include "rows_host.h"
#include "spans.h"
#include "wave.h"

#define GP_WORDS 32   // bitmap words per wavefront of gp_acgt_kernel
#define GP_SHORT 4    // a region over at most this many bitmap words is counted by its own lane

typedef unsigned long long ull;

__global__ void __launch_bounds__(256)
gp_boundary_kernel(const u32 *__restrict__ genome_off, u32 ng, ull *__restrict__ bnd) {
    const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= ng) return;
    const u32 a = genome_off[u];
    if (genome_off[u + 1] > a) atomicOr(&bnd[a >> 6], 1ull << (a & 63u));
}

// bytes: total + 256 of them (catchhip_targets::bytes), so a word's 64 lanes read inside the buffer
__global__ void __launch_bounds__(256)
gp_acgt_kernel(const u8 *__restrict__ bytes, u32 total, u32 nw, ull *__restrict__ acgt) {
    const u32 lane = threadIdx.x & 63u;
    const u32 w0 = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * GP_WORDS;
    if (w0 >= nw) return;                                   // (the whole wavefront)
    const u32 w1 = min(w0 + GP_WORDS, nw);
    for (u32 w = w0; w < w1; ++w) {
        const u64 pos = ((u64)w << 6) + lane;
        const u8 c = bytes[pos];
        const ull bits = __ballot(pos < total && (c == 'A' || c == 'C' || c == 'G' || c == 'T'));
        if (lane == 0) acgt[w] = bits;
    }
}

// the uncovered bases of word w < nw (cov: bit = depth >= min_depth; the bits from `total` on are nobody's)
__device__ __forceinline__ u64 gp_uncovered(const ull *__restrict__ cov, u32 w, u32 nw, u32 total) {
    return ~cov[w] & span_in_word((u64)w << 6, 0, total);
}

// the marks of word w < nw: bit b of *S = a region starts at base b, bit b of *E = a region's last base is b
// (bnd: nw + 1 words)
__device__ __forceinline__ void gp_marks(const ull *__restrict__ cov, const ull *__restrict__ bnd, u32 w, u32 nw,
                                         u32 total, u64 *S, u64 *E) {
    const u64 U = gp_uncovered(cov, w, nw, total);
    const u64 prev = w ? gp_uncovered(cov, w - 1, nw, total) >> 63 : 0ull;
    const u64 next = w + 1 < nw ? gp_uncovered(cov, w + 1, nw, total) & 1ull : 0ull;
    const u64 B = bnd[w];
    const u64 Bn = (B >> 1) | ((u64)bnd[w + 1] << 63);      // bit b: base b + 1 is a universe's first
    *S = U & (~((U << 1) | prev) | B);
    *E = U & (~((U >> 1) | (next << 63)) | Bn);
}

// cs[0 .. nw], ce[0 .. nw]: the marks per word, 0 behind the last word (the scans leave the totals there)
__global__ void __launch_bounds__(256)
gp_count_kernel(const ull *__restrict__ cov, const ull *__restrict__ bnd, u32 nw, u32 total, u32 *__restrict__ cs,
                u32 *__restrict__ ce) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w > nw) return;
    u64 S = 0, E = 0;
    if (w < nw) gp_marks(cov, bnd, w, nw, total, &S, &E);
    cs[w] = (u32)__popcll(S);
    ce[w] = (u32)__popcll(E);
}

// cs / ce scanned: region cs[w] + k starts at the k-th start mark of word w, region ce[w] + k ends behind the k-th
// end mark
__global__ void __launch_bounds__(256)
gp_emit_kernel(const ull *__restrict__ cov, const ull *__restrict__ bnd, u32 nw, u32 total,
               const u32 *__restrict__ cs, const u32 *__restrict__ ce, u32 nreg, u32 *__restrict__ rs,
               u32 *__restrict__ re) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nw) return;
    u64 S, E;
    gp_marks(cov, bnd, w, nw, total, &S, &E);
    const u32 base = w << 6;
    for (u32 o = cs[w]; S && o < nreg; ++o, S &= S - 1) rs[o] = base + (u32)__ffsll((ull)S) - 1u;
    for (u32 o = ce[w]; E && o < nreg; ++o, E &= E - 1) re[o] = base + (u32)__ffsll((ull)E);
}

// ua[i] = the bases of region i whose bit in acgt is set (acgt null: all of them); flag[i] = it is reported,
// flag[nreg] = 0.  Every lane of a wavefront stays to the end: the long regions are counted by all 64.
__global__ void __launch_bounds__(256)
gp_measure_kernel(const u32 *__restrict__ rs, const u32 *__restrict__ re, u32 nreg, const ull *__restrict__ acgt,
                  i64 min_length, i64 min_unambig, u32 *__restrict__ ua, u32 *__restrict__ flag) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 lane = threadIdx.x & 63u;
    const bool have = i < (i64)nreg;
    const u32 a = have ? rs[i] : 0u, b = have ? re[i] : 1u;  // (an idle lane: one base, so that it has a span)
    const u32 len = b - a;                                   // >= 1 for a region
    u32 cnt = len;
    if (acgt) {
        const bool is_long = have && span_of(a, b).nw > GP_SHORT;
        if (have && !is_long) cnt = span_popc(acgt, a, b);
        for (ull rest = __ballot(is_long); rest; rest &= rest - 1) {
            const int src = __ffsll(rest) - 1;
            const Span sp = span_of((u32)__shfl((int)a, src, WAVE), (u32)__shfl((int)b, src, WAVE));
            u32 part = 0;
            for (u32 j = lane; j < sp.nw; j += WAVE) part += span_popc_word(acgt, sp, j);
            part = wave_sum_all(part);
            if ((int)lane == src) cnt = part;
        }
    }
    if (have) {
        ua[i] = cnt;
        flag[i] = ((i64)len >= min_length && (i64)cnt >= min_unambig) ? 1u : 0u;
    } else if (i == (i64)nreg) {
        flag[i] = 0u;
    }
}

// pu[3 u .. 3 u + 2] += regions, bases; max= longest, over the reported regions of universe u
__global__ void __launch_bounds__(256)
gp_compact_kernel(const u32 *__restrict__ rs, const u32 *__restrict__ re, const u32 *__restrict__ ua,
                  const u32 *__restrict__ flag, const u32 *__restrict__ place, u32 nreg,
                  const u32 *__restrict__ genome_off, u32 ng, i32 *__restrict__ out_ua, i32 *__restrict__ out_univ,
                  u32 *__restrict__ out_gs, u32 *__restrict__ out_ge, ull *__restrict__ pu) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 lane = threadIdx.x & 63u;
    const bool on = i < (i64)nreg && flag[i];
    u32 u = 0, len = 0;
    if (on) {
        const u32 a = rs[i], b = re[i], j = place[i];
        u = find_segment(genome_off, ng, a);
        len = b - a;
        out_ua[j] = (i32)ua[i];
        out_univ[j] = (i32)u;
        out_gs[j] = a;
        out_ge[j] = b;
    }
    const ull mask = __ballot(on);
    if (!mask) return;                                       // (the whole wavefront)
    const u32 u0 = (u32)__shfl((int)u, __ffsll(mask) - 1, WAVE);
    if (__ballot(on && u != u0) == 0) {                      // one universe: one set of atomics for the wavefront
        ull bases = len;
        u32 longest = len;
        bases = wave_sum(bases);
        longest = wave_max(longest);
        if (lane == 0) {
            atomicAdd(&pu[3 * (size_t)u0], (ull)__popcll(mask));
            atomicAdd(&pu[3 * (size_t)u0 + 1], bases);
            atomicMax(&pu[3 * (size_t)u0 + 2], (ull)longest);
        }
    } else if (on) {
        atomicAdd(&pu[3 * (size_t)u], 1ull);
        atomicAdd(&pu[3 * (size_t)u + 1], (ull)len);
        atomicMax(&pu[3 * (size_t)u + 2], (ull)len);
    }
}

// cov[w] |= unwanted[w]: a base that is not wanted ends a run as a covered base does (a lane per word)
__global__ void __launch_bounds__(256)
gp_mask_kernel(const ull *__restrict__ unwanted, u32 nw, ull *__restrict__ cov) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < nw) cov[w] |= unwanted[w];
}

// catchhip_rows_uncovered (mask == null: it launches what it always launched) and catchhip_rows_uncovered_within
static int gp_rows_uncovered(catchhip_ctx *ctx, const catchhip_rows *R0, const catchhip_targets *T,
                             const catchhip_basemask *mask, i32 min_depth, i64 min_length, i64 min_unambig,
                             catchhip_rows **out, i64 *nregions, i64 *per_universe) {
    ARG_CHECK(ctx && R0 && out);
    ARG_CHECK(R0->ctx == ctx && (!T || T->ctx == ctx) && (!mask || mask->ctx == ctx));
    *out = nullptr;
    if (nregions) *nregions = 0;
    TRY(chip_rows_form_check(R0, "rows_uncovered", "the rows", true));    // (grouped rows are fine)
    if (min_depth < 1 || min_length < 1 || min_unambig < 0) {
        chip_set_error("rows_uncovered: min_depth %d, min_length %lld, min_unambig %lld; the smallest are 1, 1 and 0",
                       (int)min_depth, (long long)min_length, (long long)min_unambig);
        return CATCHHIP_EINVAL;
    }
    ARG_CHECK(R0->total >= 0 && R0->total < ((i64)1 << 32) - 4096 && R0->n >= 0 && R0->n < ((i64)1 << 31));
    const i32 ng = R0->ngenomes;
    if (T) TRY(chip_targets_space_check(T, R0, "rows_uncovered"));
    if (mask) TRY(chip_space_check(mask, R0, "rows_uncovered", "the mask is not over the coordinate space of the rows"));
    if (per_universe) for (i64 k = 0; k < 3 * (i64)ng; ++k) per_universe[k] = 0;
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DerivedRows D(ctx, R0);
    TRY(D.err);
    catchhip_rows *R = D.R.get();
    PhaseTimer &tm = D.tm;
    const u64 total = (u64)R0->total;
    if (total == 0 || ng <= 0) {                             // no bases: no regions
        TRY(D.copy_of(nullptr));
        return D.finish(out, nregions);
    }
    const u32 nw = (u32)((total + 63) >> 6), ngu = (u32)ng;
    const dim3 blk(256);
    DevBuf<ull> cov, bnd, acgt, pu;
    DevBuf<u32> cnt, scan_tmp;
    TRY(cov.alloc((size_t)nw + 2));
    TRY(bnd.alloc((size_t)nw + 2));
    TRY(cnt.alloc(2 * ((size_t)nw + 1)));
    TRY(pu.alloc(3 * (size_t)ngu));
    HIP_TRY(hipMemsetAsync(cov.p, 0, sizeof(ull) * ((size_t)nw + 2), s));
    HIP_TRY(hipMemsetAsync(bnd.p, 0, sizeof(ull) * ((size_t)nw + 2), s));
    HIP_TRY(hipMemsetAsync(pu.p, 0, sizeof(ull) * 3 * (size_t)ngu, s));
    {   // depth per base -> the bitmap of the bases at depth >= min_depth
        DevBuf<u32> d;
        TRY(chip_depth_array(ctx, R0, nullptr, 0u, nullptr, d, scan_tmp, tm));
        TRY(chip_depth_bitmap(ctx, (const u32 *)d.p, total, (u32)min_depth, (const u32 *)R0->genome_off.p, ngu, cov.p,
                              nullptr, tm));
    }
    hipLaunchKernelGGL(gp_boundary_kernel, dim3((unsigned)div_up(ngu, 256)), blk, 0, s, (const u32 *)R0->genome_off.p,
                       ngu, bnd.p);
    tm.launch(1);
    if (mask) {
        hipLaunchKernelGGL(gp_mask_kernel, dim3((unsigned)div_up(nw, 256)), blk, 0, s, (const ull *)mask->unwanted.p, nw,
                           cov.p);
        tm.launch(1);
    }
    if (T) {
        TRY(acgt.alloc((size_t)nw));
        const i64 nwaves = div_up(nw, GP_WORDS);
        hipLaunchKernelGGL(gp_acgt_kernel, dim3((unsigned)div_up(nwaves, 256 / WAVE)), blk, 0, s, (const u8 *)T->bytes.p,
                           (u32)total, nw, acgt.p);
        tm.launch(1);
    }
    u32 *cs = cnt.p, *ce = cnt.p + nw + 1;
    const dim3 per_word((unsigned)div_up((i64)nw + 1, 256));
    hipLaunchKernelGGL(gp_count_kernel, per_word, blk, 0, s, (const ull *)cov.p, (const ull *)bnd.p, nw, (u32)total, cs,
                       ce);
    TRY(chip_exclusive_scan_u32(ctx, cs, cs, (i64)nw + 1, scan_tmp));
    TRY(chip_exclusive_scan_u32(ctx, ce, ce, (i64)nw + 1, scan_tmp));
    tm.launch(3);
    HIP_TRY(hipGetLastError());
    u32 nreg = 0;                                            // sizes the region arrays: it has to come back
    TRY(read_count(ctx, cs + nw, &nreg));
    u32 nkept = 0;
    if (nreg) {
        DevBuf<u32> rs, re, ua, flag, place;
        TRY(rs.alloc(nreg));
        TRY(re.alloc(nreg));
        TRY(ua.alloc(nreg));
        TRY(flag.alloc((size_t)nreg + 1));
        TRY(place.alloc((size_t)nreg + 1));
        const dim3 per_region((unsigned)div_up((i64)nreg + 1, 256));
        hipLaunchKernelGGL(gp_emit_kernel, per_word, blk, 0, s, (const ull *)cov.p, (const ull *)bnd.p, nw, (u32)total,
                           (const u32 *)cs, (const u32 *)ce, nreg, rs.p, re.p);
        hipLaunchKernelGGL(gp_measure_kernel, per_region, blk, 0, s, (const u32 *)rs.p, (const u32 *)re.p, nreg,
                           (const ull *)acgt.p, min_length, min_unambig, ua.p, flag.p);
        TRY(chip_exclusive_scan_u32(ctx, flag.p, place.p, (i64)nreg + 1, scan_tmp));
        tm.launch(3);
        HIP_TRY(hipGetLastError());
        TRY(read_count(ctx, place.p + nreg, &nkept));
        if (nkept >= (1u << 31)) {
            chip_set_error("rows_uncovered: %u regions; a row table holds fewer than 2^31", nkept);
            return CATCHHIP_EINVAL;
        }
        if (nkept) {
            TRY(chip_rows_alloc_soa(R, nkept));
            hipLaunchKernelGGL(gp_compact_kernel, per_region, blk, 0, s, (const u32 *)rs.p, (const u32 *)re.p,
                               (const u32 *)ua.p, (const u32 *)flag.p, (const u32 *)place.p, nreg,
                               (const u32 *)R0->genome_off.p, ngu, R->set_id.p, R->univ.p, R->gs.p, R->ge.p, pu.p);
            tm.launch(1);
            HIP_TRY(hipGetLastError());
        }
    }
    tm.stop();
    std::vector<i64> h(3 * (size_t)ngu);
    TRY(chip_fetch_counters(ctx, pu.p, h.size(), h.data()));
    i64 longest = 0;
    for (size_t k = 0; k < h.size(); ++k) {
        if (per_universe) per_universe[k] = h[k];
        if (k % 3 == 2) longest = std::max(longest, h[k]);
    }
    R->n = (i64)nkept;
    R->lmax = (u32)longest;
    return D.finish(out, nregions);
}

extern "C" int catchhip_rows_uncovered(catchhip_ctx *ctx, const catchhip_rows *R0, const catchhip_targets *T,
                                       i32 min_depth, i64 min_length, i64 min_unambig, catchhip_rows **out,
                                       i64 *nregions, i64 *per_universe) {
    return gp_rows_uncovered(ctx, R0, T, nullptr, min_depth, min_length, min_unambig, out, nregions, per_universe);
}

extern "C" int catchhip_rows_uncovered_within(catchhip_ctx *ctx, const catchhip_rows *R0, const catchhip_targets *T,
                                              const catchhip_basemask *mask, i32 min_depth, i64 min_length,
                                              i64 min_unambig, catchhip_rows **out, i64 *nregions, i64 *per_universe) {
    ARG_CHECK(mask);
    return gp_rows_uncovered(ctx, R0, T, mask, min_depth, min_length, min_unambig, out, nregions, per_universe);
}
