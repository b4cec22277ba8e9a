// Rows at several cover extensions from one scan, and the grid solve built on
// them (catchhip_rows_extend, catchhip_setcover_grid).
//
// The reference extends every cover range of a probe by e on both sides,
// clips it to its sequence and normalises the ranges of a (set, universe)
// (catch/filter/set_cover_filter.py:424-453 + catch/utils/interval.py:288-316).
// A merged row of a scan at e = 0 is a run of covered bases; only the ranges at
// its two ends can reach outside it, each clipped to its own sequence.  So the
// row [s, t) at extension e is
//     s' = max(seqstart(s), s - e),   t' = min(seqend(t - 1), t + e)
// and rows whose extended ranges overlap or touch merge.  Inside a (set,
// universe) s' and t' are non-decreasing, so row r joins its predecessor
// exactly when s'_r <= t'_{r-1}, which happens from one threshold on:
//     same sequence, gap g = s_r - t_{r-1} >= 1:   ceil(g / 2)
//     sequences meeting at boundary B:            max(s_r - B, B - t_{r-1})
//     a non-empty sequence between them:          never
// One pass computes the thresholds; each e is then a flag pass (threshold > e
// starts a row), an exclusive scan of the flags and an emit.  The reference has
// no counterpart for deriving one extension from another.
#include <algorithm>
#include <chrono>

#include "rows_host.h"
#include "wave.h"

#define GRID_NEVER 0xffffffffu

// thr[r] = the smallest e at which row r merges with its predecessor (GRID_NEVER:
// first row of its (set, universe), or a whole sequence lies between the two)
__global__ void __launch_bounds__(256)
grid_thresh_kernel(const i32 *__restrict__ set_id, const i32 *__restrict__ univ, const u32 *__restrict__ gs,
                   const u32 *__restrict__ ge, u32 n, const u32 *__restrict__ seq_off, u32 nseq, u32 *__restrict__ thr) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    u32 v = GRID_NEVER;
    if (r > 0 && set_id[r] == set_id[r - 1] && univ[r] == univ[r - 1]) {
        const u32 s = gs[r], t = ge[r - 1];
        const u32 a = find_segment(seq_off, nseq, t - 1u), b = find_segment(seq_off, nseq, s);
        if (a == b) {
            v = (s - t + 1u) >> 1;                       // ceil(g / 2), g >= 1
        } else if (seq_off[a + 1] == seq_off[b]) {       // adjacent (only empty sequences between)
            const u32 B = seq_off[b];
            v = max(s - B, B - t);
        }
    }
    thr[r] = v;
}

__global__ void __launch_bounds__(256)
grid_flags_kernel(const u32 *__restrict__ thr, u32 n, u32 e, u32 *__restrict__ flag) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) flag[r] = thr[r] > e ? 1u : 0u;
}

// Row r of the e = 0 table: a head writes set, universe and the extended start of
// its output row; the last row of a run writes the extended end.  The row count
// goes to info[0].
__global__ void __launch_bounds__(256)
grid_emit_kernel(const i32 *__restrict__ set_id, const i32 *__restrict__ univ, const u32 *__restrict__ gs,
                 const u32 *__restrict__ ge, const u32 *__restrict__ thr, const u32 *__restrict__ pos, u32 n, u32 e,
                 const u32 *__restrict__ seq_off, u32 nseq, i32 *__restrict__ o_set, i32 *__restrict__ o_univ,
                 u32 *__restrict__ o_gs, u32 *__restrict__ o_ge, u32 *__restrict__ info) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const bool head = thr[r] > e;
    const bool last = r + 1 == n || thr[r + 1] > e;
    const u32 o = head ? pos[r] : pos[r] - 1u;   // (pos is exclusive; row 0 is always a head)
    if (head) {
        const u32 s = gs[r];
        const u32 lo = seq_off[find_segment(seq_off, nseq, s)];
        o_set[o] = set_id[r];
        o_univ[o] = univ[r];
        o_gs[o] = (s - lo > e) ? s - e : lo;
    }
    if (last) {
        const u32 t = ge[r];
        const u32 hi = seq_off[find_segment(seq_off, nseq, t - 1u) + 1];
        o_ge[o] = (hi - t > e) ? t + e : hi;
        if (r + 1 == n) info[0] = o + 1u;
    }
}

// per derived row: its length into gain0[set] (the first round's gains of a full-coverage solve) and the longest
// row into info[1]
__global__ void __launch_bounds__(256)
grid_len_kernel(const i32 *__restrict__ o_set, const u32 *__restrict__ o_gs, const u32 *__restrict__ o_ge, u32 cap,
                u32 *__restrict__ gain0, u32 ng, u32 *__restrict__ info) {
    const u32 o = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 n = info[0];
    u32 len = 0;
    if (o < n && o < cap) {
        len = o_ge[o] - o_gs[o];
        const u32 sid = (u32)o_set[o];
        if (gain0 && sid < ng) atomicAdd(&gain0[sid], len);
    }
    len = wave_max(len);
    if ((threadIdx.x & 63u) == 0 && len) atomicMax(&info[1], len);
}

// One derived table.  thr: thresholds of R0 (device, R0->n entries); ng = gain0 entries to fill (0: none).
static int grid_derive_one(catchhip_ctx *ctx, const catchhip_rows *R0, const catchhip_targets *T, const u32 *thr,
                           u32 e, u32 ng, DevBuf<u32> &flag, DevBuf<u32> &pos, DevBuf<u32> &scan_tmp,
                           DevBuf<u32> &info, catchhip_rows **out) {
    std::unique_ptr<catchhip_rows> R;
    TRY(chip_rows_new(ctx, R0->total, R0->ngenomes, R0->h_genome_off, R0->genome_off.p, false, R));
    R->ext = (i32)e;
    const u32 n0 = (u32)R0->n;
    hipStream_t s = ctx->stream;
    if (n0 == 0) {   // no rows to extend
        *out = R.release();
        return 0;
    }
    // (capacity n0: an extension never makes more rows, and no count has to come back before the emit)
    TRY(chip_rows_alloc_soa(R.get(), n0));
    if (ng) {
        TRY(R->gain0.alloc(ng));
        HIP_TRY(hipMemsetAsync(R->gain0.p, 0, sizeof(u32) * (size_t)ng, s));
        R->gain0_n = ng;
    }
    HIP_TRY(hipMemsetAsync(info.p, 0, sizeof(u32) * 2, s));
    const dim3 grid((unsigned)div_up(n0, 256)), blk(256);
    hipLaunchKernelGGL(grid_flags_kernel, grid, blk, 0, s, thr, n0, e, flag.p);
    TRY(chip_exclusive_scan_u32(ctx, flag.p, pos.p, n0, scan_tmp));
    hipLaunchKernelGGL(grid_emit_kernel, grid, blk, 0, s, (const i32 *)R0->set_id.p, (const i32 *)R0->univ.p,
                       (const u32 *)R0->gs.p, (const u32 *)R0->ge.p, thr, (const u32 *)pos.p, n0, e,
                       (const u32 *)T->seq_off.p, (u32)T->nseq, R->set_id.p, R->univ.p, R->gs.p, R->ge.p, info.p);
    hipLaunchKernelGGL(grid_len_kernel, grid, blk, 0, s, (const i32 *)R->set_id.p, (const u32 *)R->gs.p,
                       (const u32 *)R->ge.p, n0, ng ? R->gain0.p : (u32 *)nullptr, ng, info.p);
    HIP_TRY(hipGetLastError());
    u32 h[2];   // {rows, longest row}
    TRY(chip_read_back(ctx, info.p, sizeof(h), h));
    R->n = h[0];
    R->lmax = h[1];
    *out = R.release();
    return 0;
}

static int grid_check_rows0(const catchhip_rows *R0, const catchhip_targets *T) {
    if (R0->ext != 0) {
        chip_set_error("rows_extend: the rows were not made by a cover scan at cover_extension = 0");
        return CATCHHIP_EINVAL;
    }
    if (R0->grouped) {
        chip_set_error("rows_extend: rows of a scan with group numbers (a union of instances) are not supported");
        return CATCHHIP_EINVAL;
    }
    if (R0->deferred || R0->total != T->total || R0->ngenomes != T->ngenomes) {
        chip_set_error("rows_extend: the targets are not the ones the rows were scanned over");
        return CATCHHIP_EINVAL;
    }
    if (T->total >= ((i64)1 << 32) - 1) {
        chip_set_error("rows_extend: more than 2^32 - 2 target bases");
        return CATCHHIP_EINVAL;
    }
    return 0;
}

// the e-independent part: thresholds of every row of R0
static int grid_thresholds(catchhip_ctx *ctx, const catchhip_rows *R0, const catchhip_targets *T, DevBuf<u32> &thr) {
    TRY(thr.alloc((size_t)R0->n));
    if (R0->n == 0) return 0;
    hipLaunchKernelGGL(grid_thresh_kernel, dim3((unsigned)div_up(R0->n, 256)), dim3(256), 0, ctx->stream,
                       (const i32 *)R0->set_id.p, (const i32 *)R0->univ.p, (const u32 *)R0->gs.p, (const u32 *)R0->ge.p,
                       (u32)R0->n, (const u32 *)T->seq_off.p, (u32)T->nseq, thr.p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// what every derived table of R0 shares: the thresholds and the scratch of the flag scan
static int grid_prepare(catchhip_ctx *ctx, const catchhip_rows *R0, const catchhip_targets *T, DevBuf<u32> &thr,
                        DevBuf<u32> &flag, DevBuf<u32> &pos) {
    HIP_TRY(hipSetDevice(ctx->device));
    TRY(grid_thresholds(ctx, R0, T, thr));
    TRY(flag.alloc((size_t)R0->n));
    TRY(pos.alloc((size_t)R0->n));
    return 0;
}

extern "C" int catchhip_rows_extend(catchhip_ctx *ctx, const catchhip_rows *R0, const catchhip_targets *T,
                                    i32 n_ext, const i32 *ext, catchhip_rows **out, i64 *nrows) {
    ARG_CHECK(ctx && R0 && T && out && n_ext >= 0 && (n_ext == 0 || ext));
    ARG_CHECK(R0->ctx == ctx && T->ctx == ctx);
    for (i32 i = 0; i < n_ext; ++i) {
        out[i] = nullptr;
        if (ext[i] < 0) { chip_set_error("rows_extend: negative cover extension %d", ext[i]); return CATCHHIP_EINVAL; }
    }
    TRY(grid_check_rows0(R0, T));
    PoolScope pool_scope(ctx);
    DevBuf<u32> thr, flag, pos, scan_tmp, info;
    TRY(grid_prepare(ctx, R0, T, thr, flag, pos));
    TRY(info.alloc(2));
    for (i32 i = 0; i < n_ext; ++i) {
        const int rc = grid_derive_one(ctx, R0, T, thr.p, (u32)ext[i], R0->gain0_n, flag, pos, scan_tmp, info, &out[i]);
        if (rc) {
            for (i32 j = 0; j < i; ++j) { (void)catchhip_rows_destroy(out[j]); out[j] = nullptr; }
            return rc;
        }
        if (nrows) nrows[i] = out[i]->n;
    }
    return 0;
}

extern "C" int catchhip_rows_fetch_gain0(catchhip_ctx *ctx, const catchhip_rows *R, i64 n, u32 *gain0, i64 *n_out) {
    ARG_CHECK(ctx && R && n_out && n >= 0 && (n == 0 || gain0));
    *n_out = R->gain0_n;
    const i64 m = std::min<i64>(n, (i64)R->gain0_n);
    if (m <= 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(gain0, R->gain0.p, sizeof(u32) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int catchhip_ctx_last_grid_counters(catchhip_ctx *ctx, i64 *out4) {
    ARG_CHECK(ctx && out4);
    for (int i = 0; i < 4; ++i) out4[i] = ctx->grid_counters[i];
    return 0;
}

extern "C" int catchhip_setcover_grid(catchhip_ctx *ctx, const catchhip_probes *P, const catchhip_targets *T,
                                      i32 mismatches, i32 lcf_thres, i32 island, i32 mode, i32 n_ext, const i32 *ext,
                                      i64 num_sets, const i64 *ranks, const double *universe_p,
                                      i64 *const *out_ids, i64 *n_out, i64 *nrows) {
    ARG_CHECK(ctx && P && T && n_ext >= 0 && num_sets >= 0);
    ARG_CHECK(P->ctx == ctx && T->ctx == ctx);
    ARG_CHECK(n_ext == 0 || (ext && out_ids && n_out));
    for (i32 i = 0; i < n_ext; ++i) {
        if (ext[i] < 0) { chip_set_error("setcover_grid: negative cover extension %d", ext[i]); return CATCHHIP_EINVAL; }
        n_out[i] = 0;
        if (nrows) nrows[i] = 0;
    }
    for (int i = 0; i < 4; ++i) ctx->grid_counters[i] = 0;
    if (n_ext == 0) return 0;
    // test hook: a fresh scan at every e instead of the derivation (the two must agree)
    const bool rescan = chip_test_env_int("CATCHHIP_GRID_RESCAN", 0) != 0;
    const bool timing = getenv("CATCHHIP_TIMING") != nullptr;
    using clk = std::chrono::steady_clock;
    double scan_ms = 0.0, derive_ms = 0.0, solve_ms = 0.0;
    catchhip_rows *R0 = nullptr;
    int rc = 0;
    auto t0 = clk::now();
    if (!rescan) {
        if ((rc = catchhip_cover_scan(ctx, P, T, mismatches, lcf_thres, island, 0, mode, &R0, nullptr))) return rc;
        ctx->grid_counters[0] = 1;
        ctx->grid_counters[3] = R0->n;
        if (R0->grouped) {
            (void)catchhip_rows_destroy(R0);
            chip_set_error("setcover_grid: probes and targets with group numbers are not supported");
            return CATCHHIP_EINVAL;
        }
    }
    scan_ms += std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    {
        PoolScope pool_scope(ctx);
        DevBuf<u32> thr, flag, pos, scan_tmp, info;
        if (!rescan && R0->n) rc = grid_prepare(ctx, R0, T, thr, flag, pos);
        if (!rc && !rescan) rc = info.alloc(2);
        // the derived tables fill gain0 for every set the solver asks about (the scan's own gain0 may be missing)
        const u32 ng = (u32)std::min<i64>(std::max<i64>(num_sets, R0 ? (i64)R0->gain0_n : 0), (i64)0xfffffffe);
        // one derived table at a time: made, solved, returned to the block cache
        for (i32 i = 0; i < n_ext && !rc; ++i) {
            catchhip_rows *R = nullptr;
            auto t1 = clk::now();
            if (rescan) {
                rc = catchhip_cover_scan(ctx, P, T, mismatches, lcf_thres, island, ext[i], mode, &R, nullptr);
                ctx->grid_counters[0] += 1;
            } else {
                rc = grid_derive_one(ctx, R0, T, thr.p, (u32)ext[i], ng, flag, pos, scan_tmp, info, &R);
                ctx->grid_counters[1] += 1;
            }
            auto t2 = clk::now();
            (rescan ? scan_ms : derive_ms) += std::chrono::duration<double, std::milli>(t2 - t1).count();
            if (rc) break;
            if (nrows) nrows[i] = R->n;
            rc = catchhip_setcover_greedy(ctx, R, num_sets, ranks, universe_p, out_ids[i], &n_out[i]);
            ctx->grid_counters[2] += 1;
            solve_ms += std::chrono::duration<double, std::milli>(clk::now() - t2).count();
            (void)catchhip_rows_destroy(R);
        }
    }
    if (R0) (void)catchhip_rows_destroy(R0);
    if (timing)
        fprintf(stderr, "[catchhip] grid of %d extensions: scan %.3f ms, derive %.3f ms, solve %.3f ms (host wall)%s\n",
                n_ext, scan_ms, derive_ms, solve_ms, rescan ? " [rescan]" : "");
    return rc;
}
