// Pruning a pick list (catchhip_rows_prune): the picks that can leave a design without any base falling below its
// coverage depth D, behind SetCoverFilter(prune_redundant=True) and `python -m catch_amd.prune_probes`.
//
// The definition is a sequential walk.  depth(b) = the picked sets with a row over base b, plus the fixed rows over
// it.  The picks are examined from the last picked to the first (examination index e = npicks - 1 - position); a pick
// is removed when, at its turn, every base of its rows has depth >= D + 1, and its removal lowers those depths by 1.
// The walk is reproduced exactly, in parallel rounds:
//
//   * Depths only fall, so a pick that is not removable under the current depths never becomes removable: it is KEPT.
//   * A round's candidates are the undecided picks that are removable under the current depths.  With cand(b) = the
//     candidates over b and first(b) = the smallest examination index among them, candidate s is REMOVED in this
//     round when for each of its bases b either depth(b) - cand(b) >= D (b stays deep enough whoever leaves) or
//     first(b) == s (of the candidates over b the walk reaches s first, and nobody else over b leaves in this
//     round unless the first clause holds).  The candidate with the smallest index passes, so every round removes
//     one pick at least.  The removed picks' depths are lowered, the candidates are looked at again, and so on.
//   * A chain of picks that each conflict with the next would take a round per pick: once a round removes fewer
//     than PR_TAIL_BELOW picks, one workgroup walks the undecided picks in examination order (pr_tail_kernel).
//
//   first pass, over all `total` bases (depth.hip's steps through chip_depth_marks / _array / _bitmap):
//     marks -> difference array (picked rows + fixed rows) -> chip_exclusive_scan_u32 -> ballot bitmap of
//     depth >= D + 1 -> pr_classify_rows_kernel (a thread per row: a clear bit under a picked row keeps its set)
//     -> pr_compact_kernel (the undecided picks: the first round's candidates)
//   per round, over the candidates' rows only (a wavefront per candidate, its lanes over the bases):
//     pr_accumulate_kernel  cand[b] += 1, first[b] = min(first[b], e)       (integer atomics: order-free)
//     pr_decide_kernel      the rule above -> state[e] = REMOVED
//     pr_apply_kernel       cand / first back to their idle values; depth -= 1 under the removed picks
//     pr_recheck_kernel     undecided and still removable -> the next round's list; no longer removable -> KEPT
//   one read-back per round (the next list's length, the picks removed).
//
// Everything is integer arithmetic, and the result is the walk's whatever the launch geometry or the order of the
// atomics.  The rows of a set are contiguous in a row table of the solver's form (sorted by set): pr_ranges_kernel
// takes each set's range of rows from that and raises a flag when a set comes in two runs.
#include "rows_host.h"
#include "spans.h"
#include "wave.h"

#define PR_TAIL_BELOW 8          // a round that removes fewer picks hands the rest to the one-workgroup walk
#define PR_NONE 0xffffffffu
enum { PR_UNDECIDED = 0, PR_KEPT = 1, PR_REMOVED = 2 };

// set_of[e] = the set examined e-th; the examination index of the pick of a set is npicks - 1 - rank[set] (the pick
// table of chip_depth_marks).  The picks have passed dp_mark_kernel: in range, none twice.
__global__ void __launch_bounds__(256)
pr_order_kernel(const i64 *__restrict__ picks, u32 npicks, u32 *__restrict__ set_of) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npicks) set_of[npicks - 1 - i] = (u32)picks[i];
}

// rbeg1[s] = 1 + the first row of set s (0: no rows), rend[s] = one past its last.  flag[0] |= 4: a set in two runs
__global__ void __launch_bounds__(256)
pr_ranges_kernel(const i32 *__restrict__ set_id, u32 n, u32 num_sets, u32 *__restrict__ rbeg1, u32 *__restrict__ rend,
                 u32 *__restrict__ flag) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const i32 s = set_id[r];
    if ((u32)s >= num_sets) return;
    if (r == 0 || set_id[r - 1] != s) {
        if (atomicExch(&rbeg1[s], r + 1)) atomicOr(&flag[0], 4u);
    }
    if (r == n - 1 || set_id[r + 1] != s) rend[s] = r + 1;
}

// bm bit b = depth(b) >= D + 1.  A row of a picked set with a clear bit under it: the set is not removable
__global__ void __launch_bounds__(256)
pr_classify_rows_kernel(const i32 *__restrict__ set_id, const u32 *__restrict__ gs, const u32 *__restrict__ ge, u32 n,
                        u32 num_sets, const u32 *__restrict__ rank, u32 npicks,
                        const unsigned long long *__restrict__ bm, u32 *__restrict__ state) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const u32 s = (u32)set_id[r];
    if (s >= num_sets) return;
    const u32 rk = rank[s];
    if (rk == CHIP_NOT_PICKED) return;
    const u32 a = gs[r], b = ge[r];
    if (b > a && !span_all_set(bm, a, b)) state[npicks - 1 - rk] = PR_KEPT;
}

// list[0 .. ctr[0]) = the undecided picks (examination indices, any order); a thread per pick, one atomic per wavefront
__global__ void __launch_bounds__(256)
pr_compact_kernel(const u32 *__restrict__ state, u32 npicks, u32 *__restrict__ list, u32 *__restrict__ ctr) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 lane = threadIdx.x & 63u;
    const bool take = e < npicks && state[e] == PR_UNDECIDED;
    const unsigned long long mask = __ballot(take);
    if (!mask) return;                                       // (the whole wavefront)
    u32 base = 0;
    if (lane == 0) base = atomicAdd(&ctr[0], (u32)__popcll(mask));
    base = (u32)__shfl((int)base, 0, WAVE);
    if (take) list[base + (u32)__popcll(mask & ((1ull << lane) - 1ull))] = e;
}

// One candidate's bases: f(b) for every base b of every row of set s, the wavefront's lanes side by side
template <typename F>
__device__ __forceinline__ void pr_for_bases(u32 s, const u32 *__restrict__ rbeg1, const u32 *__restrict__ rend,
                                             const u32 *__restrict__ gs, const u32 *__restrict__ ge, u32 lane,
                                             u32 stride, F f) {
    const u32 r0 = rbeg1[s];
    if (!r0) return;
    const u32 r1 = rend[s];
    for (u32 r = r0 - 1; r < r1; ++r) {
        const u32 a = gs[r], b1 = ge[r], len = b1 > a ? b1 - a : 0u;
        for (u32 o = lane; o < len; o += stride) f(a + o);   // (offsets: a + o stays below 2^32 - 1)
    }
}

__global__ void __launch_bounds__(256)
pr_accumulate_kernel(const u32 *__restrict__ list, u32 ncand, const u32 *__restrict__ set_of,
                     const u32 *__restrict__ rbeg1, const u32 *__restrict__ rend, const u32 *__restrict__ gs,
                     const u32 *__restrict__ ge, u32 *__restrict__ cand, u32 *__restrict__ first) {
    const u32 i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (i >= ncand) return;                                  // (the whole wavefront)
    const u32 e = list[i];
    pr_for_bases(set_of[e], rbeg1, rend, gs, ge, lane, WAVE, [&](u32 b) {
        atomicAdd(&cand[b], 1u);
        atomicMin(&first[b], e);
    });
}

// dep[b + 1] = depth(b).  ctr[1] += the picks removed
__global__ void __launch_bounds__(256)
pr_decide_kernel(const u32 *__restrict__ list, u32 ncand, const u32 *__restrict__ set_of,
                 const u32 *__restrict__ rbeg1, const u32 *__restrict__ rend, const u32 *__restrict__ gs,
                 const u32 *__restrict__ ge, const u32 *__restrict__ dep, const u32 *__restrict__ cand,
                 const u32 *__restrict__ first, u32 D, u32 *__restrict__ state, u32 *__restrict__ ctr) {
    const u32 i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (i >= ncand) return;                                  // (the whole wavefront)
    const u32 e = list[i];
    bool ok = true;
    pr_for_bases(set_of[e], rbeg1, rend, gs, ge, lane, WAVE, [&](u32 b) {
        // (every candidate over b counts in dep: dep >= cand)
        ok = ok && (dep[b + 1] - cand[b] >= D || first[b] == e);
    });
    if (__ballot(!ok) == 0ull && lane == 0) {
        state[e] = PR_REMOVED;
        atomicAdd(&ctr[1], 1u);
    }
}

__global__ void __launch_bounds__(256)
pr_apply_kernel(const u32 *__restrict__ list, u32 ncand, const u32 *__restrict__ set_of,
                const u32 *__restrict__ rbeg1, const u32 *__restrict__ rend, const u32 *__restrict__ gs,
                const u32 *__restrict__ ge, const u32 *__restrict__ state, u32 *__restrict__ dep,
                u32 *__restrict__ cand, u32 *__restrict__ first) {
    const u32 i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (i >= ncand) return;                                  // (the whole wavefront)
    const u32 e = list[i];
    const bool gone = state[e] == PR_REMOVED;
    pr_for_bases(set_of[e], rbeg1, rend, gs, ge, lane, WAVE, [&](u32 b) {
        cand[b] = 0u;                                        // (several candidates may store the same idle values)
        first[b] = PR_NONE;
        if (gone) atomicSub(&dep[b + 1], 1u);
    });
}

// next[0 .. ctr[0]) = the candidates that are undecided and removable under the lowered depths; the others that are
// undecided are kept for good
__global__ void __launch_bounds__(256)
pr_recheck_kernel(const u32 *__restrict__ list, u32 ncand, const u32 *__restrict__ set_of,
                  const u32 *__restrict__ rbeg1, const u32 *__restrict__ rend, const u32 *__restrict__ gs,
                  const u32 *__restrict__ ge, const u32 *__restrict__ dep, u32 D, u32 *__restrict__ state,
                  u32 *__restrict__ next, u32 *__restrict__ ctr) {
    const u32 i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (i >= ncand) return;                                  // (the whole wavefront)
    const u32 e = list[i];
    if (state[e] != PR_UNDECIDED) return;                    // (uniform over the wavefront)
    bool ok = true;
    pr_for_bases(set_of[e], rbeg1, rend, gs, ge, lane, WAVE, [&](u32 b) { ok = ok && dep[b + 1] > D; });
    const bool all = __ballot(!ok) == 0ull;
    if (lane == 0) {
        if (all) next[atomicAdd(&ctr[0], 1u)] = e;
        else state[e] = PR_KEPT;
    }
}

// The walk itself, by ONE workgroup, over the picks that are still undecided: in examination order, a pick whose
// bases all lie at depth >= D + 1 is removed and its bases' depths lowered (the rows of one set do not overlap: plain
// stores).  dep is read and written by all threads between barriers, hence no __restrict__ on it.  ctr[1] = the picks
// removed here.
__global__ void __launch_bounds__(256)
pr_tail_kernel(const u32 *__restrict__ set_of, u32 npicks, const u32 *__restrict__ rbeg1,
               const u32 *__restrict__ rend, const u32 *__restrict__ gs, const u32 *__restrict__ ge, u32 D, u32 *dep,
               u32 *state, u32 *__restrict__ ctr) {
    __shared__ unsigned long long undecided[256 / WAVE];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    u32 removed = 0;
    for (u32 base = 0; base < npicks; base += 256) {
        const u32 mine = base + tid;
        const unsigned long long mask = __ballot(mine < npicks && state[mine] == PR_UNDECIDED);
        if (lane == 0) undecided[wave] = mask;
        __syncthreads();
        for (u32 w = 0; w < 256 / WAVE; ++w) {
            u64 m = undecided[w];                            // (the same in every thread)
            while (m) {
                const u32 e = base + w * WAVE + (u32)__builtin_ctzll(m);
                m &= m - 1;
                const u32 s = set_of[e];
                bool low = false;
                pr_for_bases(s, rbeg1, rend, gs, ge, tid, 256u, [&](u32 b) { low = low || dep[b + 1] <= D; });
                const bool keep = __syncthreads_or(low) != 0;
                if (!keep) {
                    pr_for_bases(s, rbeg1, rend, gs, ge, tid, 256u, [&](u32 b) { dep[b + 1] -= 1u; });
                    ++removed;
                }
                if (tid == 0) state[e] = keep ? PR_KEPT : PR_REMOVED;
                __syncthreads();                             // the lowered depths, before the next pick reads them
            }
        }
        __syncthreads();                                     // (undecided[] is rewritten)
    }
    if (tid == 0) ctr[1] = removed;
}

// out[i] = the pick at position i was removed
__global__ void __launch_bounds__(256)
pr_flags_kernel(const u32 *__restrict__ state, u32 npicks, u8 *__restrict__ out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npicks) out[i] = state[npicks - 1 - i] == PR_REMOVED;
}

extern "C" int catchhip_rows_prune(catchhip_ctx *ctx, const catchhip_rows *R0, const catchhip_rows *F, i64 num_sets,
                                   const i64 *picks, i64 npicks, i32 depth, u8 *removed_flags, i64 *nremoved,
                                   i64 *rounds) {
    ARG_CHECK(ctx && R0);
    ARG_CHECK(R0->ctx == ctx);
    if (nremoved) *nremoved = 0;
    if (rounds) *rounds = 0;
    ARG_CHECK(num_sets >= 0 && num_sets < ((i64)1 << 31) && npicks >= 0 && (npicks == 0 || (picks && removed_flags)));
    TRY(chip_depth_check(R0, num_sets, npicks, depth, "rows_prune"));
    if (F) {
        if (F->ctx != ctx) {
            chip_set_error("rows_prune: the fixed rows belong to another context");
            return CATCHHIP_EINVAL;
        }
        TRY(chip_rows_form_check(F, "rows_prune", "the fixed rows"));
        TRY(chip_space_check(F, R0, "rows_prune", "the fixed rows are not over the coordinate space of the rows"));
        TRY(chip_rows_limits_check("rows_prune", F->total, F->n));
    }
    if (npicks == 0) return 0;
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    PhaseTimer tm(ctx, PHASE_ROWS);
    const u32 np = (u32)npicks, ns = (u32)num_sets, n0 = (u32)R0->n;
    const u64 total = (u64)R0->total;
    DevBuf<i64> d_picks;
    DevBuf<u32> rank;
    DevBuf<u8> picked;
    TRY(chip_depth_marks(ctx, picks, npicks, num_sets, d_picks, rank, picked, tm, "rows_prune"));
    if (n0 == 0 || total == 0) {                             // no pick has a row: each covers nothing alone
        memset(removed_flags, 1, (size_t)npicks);
        if (nremoved) *nremoved = npicks;
        tm.finish();
        return 0;
    }
    // examination order, every set's range of rows, the depth array and the bitmap of depth >= D + 1
    DevBuf<u32> set_of, rbeg1, rend, state, flag, ctr, list, next, dep, scan_tmp, cand, first;
    DevBuf<unsigned long long> bm;
    const u32 D = (u32)depth;
    TRY(set_of.alloc(np));
    TRY(rbeg1.alloc(ns));
    TRY(rend.alloc(ns));
    TRY(state.alloc(np));
    TRY(flag.alloc(1));
    TRY(ctr.alloc(2));
    TRY(list.alloc(np));
    TRY(next.alloc(np));
    TRY(chip_cut_bitmap(ctx, R0->total, true, bm));
    HIP_TRY(hipMemsetAsync(rbeg1.p, 0, sizeof(u32) * (size_t)ns, s));
    HIP_TRY(hipMemsetAsync(rend.p, 0, sizeof(u32) * (size_t)ns, s));
    HIP_TRY(hipMemsetAsync(state.p, 0, sizeof(u32) * (size_t)np, s));
    HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(u32), s));
    HIP_TRY(hipMemsetAsync(ctr.p, 0, sizeof(u32) * 2, s));
    const dim3 blk(256), per_pick((unsigned)div_up(np, 256)), per_row((unsigned)div_up(n0, 256));
    hipLaunchKernelGGL(pr_order_kernel, per_pick, blk, 0, s, (const i64 *)d_picks.p, np, set_of.p);
    hipLaunchKernelGGL(pr_ranges_kernel, per_row, blk, 0, s, (const i32 *)R0->set_id.p, n0, ns, rbeg1.p, rend.p, flag.p);
    tm.launch(2);
    TRY(chip_depth_array(ctx, R0, (const u8 *)picked.p, ns, F, dep, scan_tmp, tm));
    TRY(chip_depth_bitmap(ctx, (const u32 *)dep.p, total, D + 1u, (const u32 *)R0->genome_off.p, (u32)R0->ngenomes, bm.p,
                          nullptr, tm));
    hipLaunchKernelGGL(pr_classify_rows_kernel, per_row, blk, 0, s, (const i32 *)R0->set_id.p, (const u32 *)R0->gs.p,
                       (const u32 *)R0->ge.p, n0, ns, (const u32 *)rank.p, np, (const unsigned long long *)bm.p, state.p);
    hipLaunchKernelGGL(pr_compact_kernel, per_pick, blk, 0, s, (const u32 *)state.p, np, list.p, ctr.p);
    tm.launch(2);
    HIP_TRY(hipGetLastError());
    u32 h_flag = 0, h_ctr[2] = {0, 0};
    TRY(read_count(ctx, flag.p, &h_flag));
    if (h_flag) {
        chip_set_error("rows_prune: the rows of a set are not contiguous (the table is not sorted by set)");
        return CATCHHIP_EINVAL;
    }
    TRY(chip_read_back(ctx, ctr.p, sizeof(h_ctr), h_ctr));
    u32 ncand = h_ctr[0];
    i64 nrounds = 0;
    if (ncand) {
        // cand / first per base: idle (0 / PR_NONE) between rounds, touched under the candidates' rows only
        TRY(cand.alloc(total + 1));
        TRY(first.alloc(total + 1));
        HIP_TRY(hipMemsetAsync(cand.p, 0, sizeof(u32) * (total + 1), s));
        HIP_TRY(hipMemsetAsync(first.p, 0xff, sizeof(u32) * (total + 1), s));
    }
    const u32 *rb = rbeg1.p, *re = rend.p, *so = set_of.p, *gs = R0->gs.p, *ge = R0->ge.p;
    while (ncand) {
        ++nrounds;
        const dim3 grid((unsigned)div_up(ncand, 256 / WAVE));
        HIP_TRY(hipMemsetAsync(ctr.p, 0, sizeof(u32) * 2, s));
        hipLaunchKernelGGL(pr_accumulate_kernel, grid, blk, 0, s, (const u32 *)list.p, ncand, so, rb, re, gs, ge, cand.p,
                           first.p);
        hipLaunchKernelGGL(pr_decide_kernel, grid, blk, 0, s, (const u32 *)list.p, ncand, so, rb, re, gs, ge,
                           (const u32 *)dep.p, (const u32 *)cand.p, (const u32 *)first.p, D, state.p, ctr.p);
        hipLaunchKernelGGL(pr_apply_kernel, grid, blk, 0, s, (const u32 *)list.p, ncand, so, rb, re, gs, ge,
                           (const u32 *)state.p, dep.p, cand.p, first.p);
        hipLaunchKernelGGL(pr_recheck_kernel, grid, blk, 0, s, (const u32 *)list.p, ncand, so, rb, re, gs, ge,
                           (const u32 *)dep.p, D, state.p, next.p, ctr.p);
        tm.launch(4);
        HIP_TRY(hipGetLastError());
        TRY(chip_read_back(ctx, ctr.p, sizeof(h_ctr), h_ctr));
        if (h_ctr[1] == 0 || h_ctr[0] > ncand) {             // (the first candidate of the walk always passes)
            chip_set_error("rows_prune: a round of %u candidates removed %u and left %u", ncand, h_ctr[1], h_ctr[0]);
            return CATCHHIP_EINVAL;
        }
        list.swap(next);
        ncand = h_ctr[0];
        if (ncand && h_ctr[1] < PR_TAIL_BELOW) {
            ++nrounds;
            hipLaunchKernelGGL(pr_tail_kernel, dim3(1), blk, 0, s, so, np, rb, re, gs, ge, D, dep.p, state.p, ctr.p);
            tm.launch(1);
            HIP_TRY(hipGetLastError());
            ncand = 0;
        }
    }
    DevBuf<u8> flags;
    TRY(flags.alloc(np));
    hipLaunchKernelGGL(pr_flags_kernel, per_pick, blk, 0, s, (const u32 *)state.p, np, flags.p);
    tm.launch(1);
    HIP_TRY(hipGetLastError());
    tm.stop();
    TRY(chip_pinned_reserve(ctx, (size_t)np));
    HIP_TRY(hipMemcpyAsync(ctx->h_big, flags.p, (size_t)np, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(removed_flags, ctx->h_big, (size_t)np);
    tm.finish();
    i64 gone = 0;
    for (i64 i = 0; i < npicks; ++i) gone += removed_flags[i] != 0;
    if (nremoved) *nremoved = gone;
    if (rounds) *rounds = nrounds;
    return 0;
}
