// Rows below a coverage depth (catchhip_rows_below_depth): the reduced set cover instance of one layer of
// SetCoverFilter(coverage_depth=D).
//
// Layer k of the layered greedy asks for every base to lie in k picked sets.  The sets picked by the layers before
// it are out of the running, and a base that k of them hold already needs nothing more: the layer's instance is the
// rows of the unpicked sets, each cut into its maximal runs of bases at depth < k, where depth(b) = the number of
// picked sets with a row over b.  The rows of one set never overlap, so that is the number of picked ROWS over b.
//
//   1. dp_mark_kernel       the pick table: rank[set] = the pick's position, picked[set] = 1; a set named twice or out
//                           of range raises a flag
//   2. dp_diff_kernel       over the picked rows: span_mark_diff (spans.h)
//   3. chip_exclusive_scan_u32 in place: depth[b] = d[b + 1].  A row never leaves its universe, so the depth falls
//                           to 0 at every universe boundary and one scan serves the whole coordinate space.
//   4. dp_threshold_kernel  a lane per base: __ballot(depth >= k) is one 64-bit word of the bitmap of bases that need
//                           nothing more; lane 0 stores it and adds its bits to reached[universe]
//   5. chip_rows_cut        subtract.hip's count, scan and emit over that bitmap, the picked sets left out whole
//
// Everything is integer arithmetic.  Steps 1 to 4 are also host calls of their own (chip_depth_marks, chip_depth_array,
// chip_depth_bitmap; rows_host.h): catchhip_rows_prune (prune.hip) starts from the same depth array and bitmap,
// catchhip_rows_pick_gains (gains.hip) from the pick table, catchhip_rows_window_depth (analysis.hip) from step 2.
#include "rows_host.h"
#include "spans.h"
#include "wave.h"

#define DP_WORDS 32   // bitmap words (of 64 bases) per wavefront of dp_threshold_kernel: one atomic per wave and universe

// rank / picked: all ones / zero beforehand.  flag[0] |= 1: an id outside [0, num_sets); |= 2: an id given twice
__global__ void __launch_bounds__(256)
dp_mark_kernel(const i64 *__restrict__ picks, u32 npicks, i64 num_sets, u32 *__restrict__ rank, u8 *__restrict__ picked,
               u32 *__restrict__ flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npicks) return;
    const i64 s = picks[i];
    if (s < 0 || s >= num_sets) { atomicOr(&flag[0], 1u); return; }
    if (atomicCAS(&rank[s], CHIP_NOT_PICKED, i) != CHIP_NOT_PICKED) atomicOr(&flag[0], 2u);
    picked[s] = 1;
}

// the rows of the picked sets (picked == null: every row) on the difference array d; empty rows leave no mark
__global__ void __launch_bounds__(256)
dp_diff_kernel(const i32 *__restrict__ set_id, const u32 *__restrict__ gs, const u32 *__restrict__ ge, u32 n,
               const u8 *__restrict__ picked, u32 num_sets, u32 *__restrict__ d) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    if (picked && ((u32)set_id[r] >= num_sets || !picked[(u32)set_id[r]])) return;
    const u32 a = gs[r], b = ge[r];
    if (b > a) span_mark_diff(d, a, b);
}

// d[b + 1] = depth of base b.  Wavefront v takes the words [v * DP_WORDS, (v + 1) * DP_WORDS) of the bitmap, lowest
// first: bit b of bm = depth(b) >= k.  Lane 0 keeps the universe the walk is in and the bits it counted there, and
// adds them to reached[] (may be null: nobody counts) when the walk leaves the universe (boundaries are not
// word-aligned) and at the end.
__global__ void __launch_bounds__(256)
dp_threshold_kernel(const u32 *__restrict__ d, u32 total, u32 k, const u32 *__restrict__ genome_off, u32 ng,
                    unsigned long long *__restrict__ bm, unsigned long long *__restrict__ reached) {
    const u32 lane = threadIdx.x & 63u;
    const u32 nw = (u32)(((u64)total + 63) >> 6);
    const u32 w0 = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * DP_WORDS;
    if (w0 >= nw) return;                                   // (the whole wavefront)
    const u32 w1 = min(w0 + DP_WORDS, nw);
    u32 u = 0;
    u64 uend = 0;
    unsigned long long acc = 0;
    if (lane == 0) {
        u = find_segment(genome_off, ng, w0 << 6);
        uend = genome_off[u + 1];
    }
    for (u32 w = w0; w < w1; ++w) {
        const u64 pos = ((u64)w << 6) + lane;
        const bool in = pos < total && d[pos + 1] >= k;
        const unsigned long long bits = __ballot(in);
        if (lane == 0) {
            bm[w] = bits;
            const u64 base = (u64)w << 6;
            u64 rest = bits;
            while (rest) {
                if (uend >= base + 64 || u + 1 >= ng) {     // the rest of the word lies in universe u
                    acc += (u32)__popcll(rest);
                    break;
                }
                const u64 m = uend > base ? span_in_word(base, base, uend) : 0ull;    // universe u's bits: 63 at most
                acc += (u32)__popcll(rest & m);
                rest &= ~m;
                if (rest) {                                 // on to the next universe
                    if (acc && reached) atomicAdd(&reached[u], acc);
                    acc = 0;
                    ++u;
                    uend = genome_off[u + 1];
                }
            }
        }
    }
    if (lane == 0 && acc && reached) atomicAdd(&reached[u], acc);
}

// ---- the steps above as host calls (rows_host.h) ---------------------------------------------------------------------
int chip_depth_marks(catchhip_ctx *ctx, const i64 *picks, i64 npicks, i64 num_sets, DevBuf<i64> &d_picks,
                     DevBuf<u32> &rank, DevBuf<u8> &picked, PhaseTimer &tm, const char *who) {
    hipStream_t s = ctx->stream;
    DevBuf<u32> flag;
    TRY(d_picks.alloc((size_t)npicks));
    TRY(rank.alloc((size_t)num_sets));
    TRY(picked.alloc((size_t)num_sets));
    TRY(flag.alloc(1));
    HIP_TRY(hipMemcpyAsync(d_picks.p, picks, sizeof(i64) * (size_t)npicks, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(rank.p, 0xff, sizeof(u32) * (size_t)num_sets, s));
    HIP_TRY(hipMemsetAsync(picked.p, 0, (size_t)num_sets, s));
    HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(u32), s));
    hipLaunchKernelGGL(dp_mark_kernel, dim3((unsigned)div_up(npicks, 256)), dim3(256), 0, s, (const i64 *)d_picks.p,
                       (u32)npicks, num_sets, rank.p, picked.p, flag.p);
    tm.launch(1);
    HIP_TRY(hipGetLastError());
    u32 h_flag = 0;
    TRY(read_count(ctx, flag.p, &h_flag));                   // (also: the pageable picks[] has been read)
    if (h_flag) {
        chip_set_error("%s: a pick %s", who, (h_flag & 1u) ? "lies outside the set ids" : "is given twice");
        return CATCHHIP_EINVAL;
    }
    return 0;
}

// the one difference kernel over the rows of R (picked null: all of them); returns its launches, 0 for an empty table
i64 chip_depth_diff(catchhip_ctx *ctx, const catchhip_rows *R, const u8 *picked, u32 num_sets, u32 *d) {
    if (!R->n) return 0;
    hipLaunchKernelGGL(dp_diff_kernel, dim3((unsigned)div_up(R->n, 256)), dim3(256), 0, ctx->stream,
                       (const i32 *)R->set_id.p, (const u32 *)R->gs.p, (const u32 *)R->ge.p, (u32)R->n, picked, num_sets, d);
    return 1;
}

// d[b + 1] = the picked rows of R0 over base b, plus the rows of F (may be null: none) over it; total + 2 entries
int chip_depth_array(catchhip_ctx *ctx, const catchhip_rows *R0, const u8 *picked, u32 num_sets, const catchhip_rows *F,
                     DevBuf<u32> &d, DevBuf<u32> &tmp, PhaseTimer &tm) {
    hipStream_t s = ctx->stream;
    const u64 total = (u64)R0->total;
    TRY(d.alloc(total + 2));
    TRY(chip_exclusive_scan_reserve(tmp, (i64)total + 1));
    HIP_TRY(hipMemsetAsync(d.p, 0, sizeof(u32) * (total + 2), s));
    tm.launch(chip_depth_diff(ctx, R0, picked, num_sets, d.p));
    if (F) tm.launch(chip_depth_diff(ctx, F, nullptr, 0u, d.p));
    TRY(chip_exclusive_scan_u32(ctx, d.p, d.p, (i64)total + 1, tmp));
    tm.launch(1);
    HIP_TRY(hipGetLastError());
    return 0;
}

// bit b of bm (zeroed by the caller) = d[b + 1] >= k; reached[u] (device, zeroed by the caller; may be null) += the
// bits of universe u
int chip_depth_bitmap(catchhip_ctx *ctx, const u32 *d, u64 total, u32 k, const u32 *genome_off, u32 ng,
                      unsigned long long *bm, unsigned long long *reached, PhaseTimer &tm) {
    const u64 nwaves = div_up((i64)div_up((i64)total, 64), DP_WORDS);
    hipLaunchKernelGGL(dp_threshold_kernel, dim3((unsigned)div_up((i64)nwaves, 256 / WAVE)), dim3(256), 0, ctx->stream,
                       d, (u32)total, k, genome_off, ng, bm, reached);
    tm.launch(1);
    HIP_TRY(hipGetLastError());
    return 0;
}

// (R0 passed ARG_CHECK)
int chip_depth_check(const catchhip_rows *R0, i64 num_sets, i64 npicks, i32 depth, const char *who) {
    if (depth < 1) {
        chip_set_error("%s: depth %d; the smallest depth is 1", who, (int)depth);
        return CATCHHIP_EINVAL;
    }
    TRY(chip_rows_form_check(R0, who, "the rows"));
    TRY(chip_rows_limits_check(who, R0->total, R0->n));
    if (npicks > num_sets) {
        chip_set_error("%s: %lld picks of %lld sets (an id is repeated or out of range)", who,
                       (long long)npicks, (long long)num_sets);
        return CATCHHIP_EINVAL;
    }
    return 0;
}

extern "C" int catchhip_rows_below_depth(catchhip_ctx *ctx, const catchhip_rows *R0, i64 num_sets, const i64 *picks,
                                         i64 npicks, i32 depth, catchhip_rows **out, i64 *nrows, i64 *reached) {
    ARG_CHECK(ctx && R0 && out);
    ARG_CHECK(R0->ctx == ctx);
    *out = nullptr;
    if (nrows) *nrows = 0;
    ARG_CHECK(num_sets >= 0 && num_sets < ((i64)1 << 31) && npicks >= 0 && (npicks == 0 || picks));
    TRY(chip_depth_check(R0, num_sets, npicks, depth, "rows_below_depth"));
    const i32 ng = R0->ngenomes;
    if (reached) for (i32 u = 0; u < ng; ++u) reached[u] = 0;
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DerivedRows D(ctx, R0);
    TRY(D.err);
    catchhip_rows *R = D.R.get();
    if (npicks == 0) {                                       // depth 0 everywhere: a copy, nothing reached
        TRY(D.copy_of(R0));
        return D.finish(out, nrows);
    }
    // the picked sets (their ranks are not needed here)
    DevBuf<i64> d_picks;
    DevBuf<u32> rank;
    DevBuf<u8> picked;
    TRY(chip_depth_marks(ctx, picks, npicks, num_sets, d_picks, rank, picked, D.tm, "rows_below_depth"));
    // depth per base -> the bitmap of bases at depth >= `depth`, and their number per universe
    const u64 total = (u64)R0->total;
    DevBuf<unsigned long long> bm, d_reached;
    TRY(chip_cut_bitmap(ctx, R0->total, true, bm));
    TRY(d_reached.alloc((size_t)ng));
    HIP_TRY(hipMemsetAsync(d_reached.p, 0, sizeof(unsigned long long) * (size_t)(ng ? ng : 1), s));
    if (R0->n && total && ng > 0) {
        DevBuf<u32> d, tmp;
        TRY(chip_depth_array(ctx, R0, (const u8 *)picked.p, (u32)num_sets, nullptr, d, tmp, D.tm));
        TRY(chip_depth_bitmap(ctx, (const u32 *)d.p, total, (u32)depth, (const u32 *)R0->genome_off.p, (u32)ng, bm.p,
                              d_reached.p, D.tm));
        TRY(chip_rows_cut(ctx, R0, (const unsigned long long *)bm.p, (const u8 *)picked.p, (u32)num_sets, R, D.tm,
                          "rows_below_depth"));
    }
    if (R->n == 0 && R0->gain0_n) {                          // nothing left of any set: gain0 is carried all the same
        TRY(R->gain0.alloc(R0->gain0_n));
        HIP_TRY(hipMemsetAsync(R->gain0.p, 0, sizeof(u32) * (size_t)R0->gain0_n, s));
        R->gain0_n = R0->gain0_n;
    }
    D.tm.stop();
    TRY(chip_fetch_counters(ctx, d_reached.p, (size_t)(ng > 0 ? ng : 0), reached));
    return D.finish(out, nrows);
}
