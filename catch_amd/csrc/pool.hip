// The pooling step: one designed grid point per dataset, minimum loss, total
// probe count within a budget (catchhip_pool_solve).
//
// The reference relaxes the choice to continuous parameters, interpolates probe
// counts between grid points, minimises loss + a logarithmic barrier with
// scipy's fmin_tnc from a random start and rounds the result back to a grid
// (catch/pool/param_search.py:25-126, :268-318, :362-520, :547-658).  Over
// designed points only the problem is a multiple-choice knapsack with an exact
// answer:
//     f_0[b] = 0,   f_i[b] = min over k with n_ik <= b of f_{i-1}[b - n_ik] + l_ik
// in float64, +inf where no option fits, the smallest k among equal values; the
// answer is f_D[B] traced back from b = B.  One launch per dataset, one lane per
// budget cell: every cell of a step is independent of the others.  The cell
// reads f_{i-1} at K shifted places (a wave reads K contiguous 512-byte runs of
// an array of a few megabytes) and writes f_i[b] and a 16-bit choice; the
// D x (B + 1) choice table stays on the device and a one-lane launch walks it
// back, so only D indices return to the host.
#include <algorithm>
#include <cmath>
#include <limits>

#include "internal.h"

#define POOL_BLOCK 256
#define POOL_STAGE 1024          // options staged in LDS at a time (12 KiB)
#define POOL_NO_CHOICE 0xffffu   // f_i[b] = +inf: no option fits

// f_i[b] and choice_i[b] for cell b = the global thread index.  cnt[] holds min(n, B + 1): an option that can
// never fit compares greater than every b.
__global__ void __launch_bounds__(POOL_BLOCK)
pool_step_kernel(const double *__restrict__ f_prev, double *__restrict__ f_cur, uint16_t *__restrict__ choice,
                 const u32 *__restrict__ cnt, const double *__restrict__ loss, u32 K, u32 ncell) {
    __shared__ u32 s_cnt[POOL_STAGE];
    __shared__ double s_loss[POOL_STAGE];
    const u32 b = blockIdx.x * POOL_BLOCK + threadIdx.x;
    const bool live = b < ncell;
    double best = INFINITY;
    u32 best_k = POOL_NO_CHOICE;
    for (u32 k0 = 0; k0 < K; k0 += POOL_STAGE) {
        const u32 m = min((u32)POOL_STAGE, K - k0);
        if (k0) __syncthreads();
        for (u32 j = threadIdx.x; j < m; j += POOL_BLOCK) {
            s_cnt[j] = cnt[k0 + j];
            s_loss[j] = loss[k0 + j];
        }
        __syncthreads();
        if (live) {
#pragma unroll 4
            for (u32 j = 0; j < m; ++j) {
                const u32 n = s_cnt[j];
                if (n <= b) {
                    const double v = f_prev[b - n] + s_loss[j];
                    if (v < best) { best = v; best_k = k0 + j; }     // strict: the smallest k keeps a tie
                }
            }
        }
    }
    if (live) {
        f_cur[b] = best;
        choice[b] = (uint16_t)best_k;
    }
}

// The D dependent steps of the walk back from b = B, one lane.  The host has checked that the budget can be met, so
// f_D[B] is finite and every cell on the walk holds a choice with n <= b.  res[0] = total count, res[1] = f_D[B]'s bits.
__global__ void pool_trace_kernel(const uint16_t *__restrict__ choice, const u32 *__restrict__ cnt,
                                  const i64 *__restrict__ opt_off, i64 D, u32 ncell, const double *__restrict__ f_last,
                                  i32 *__restrict__ out_choice, unsigned long long *__restrict__ res) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    u32 b = ncell - 1;
    for (i64 i = D - 1; i >= 0; --i) {
        const u32 k = choice[(size_t)i * ncell + b];
        out_choice[i] = (i32)k;
        b -= cnt[opt_off[i] + k];
    }
    res[0] = (unsigned long long)(ncell - 1 - b);
    res[1] = (unsigned long long)__double_as_longlong(f_last[ncell - 1]);
}

extern "C" int catchhip_pool_solve(catchhip_ctx *ctx, i64 D, const i64 *opt_off, const i64 *counts,
                                   const double *losses, i64 budget, i32 *out_choice, i64 *out_total,
                                   double *out_loss) {
    ARG_CHECK(ctx && D >= 0 && opt_off && out_total && out_loss && (D == 0 || (counts && losses && out_choice)));
    ARG_CHECK(opt_off[0] == 0);
    if (budget < 0) { chip_set_error("pool_solve: negative budget %lld", (long long)budget); return CATCHHIP_EINVAL; }
    i64 kmax = 0, sum_min = 0, sum_max = 0;
    for (i64 i = 0; i < D; ++i) {
        const i64 nopt = opt_off[i + 1] - opt_off[i];
        if (nopt <= 0) {
            chip_set_error("pool_solve: dataset %lld has no options", (long long)i);
            return CATCHHIP_EINVAL;
        }
        if (nopt > 65535) {
            chip_set_error("pool_solve: dataset %lld has %lld options; the choice table holds at most 65535 per dataset",
                           (long long)i, (long long)nopt);
            return CATCHHIP_EINVAL;
        }
        kmax = std::max(kmax, nopt);
        i64 lo = std::numeric_limits<i64>::max(), hi = 0;
        for (i64 j = opt_off[i]; j < opt_off[i + 1]; ++j) {
            if (counts[j] < 0) {
                chip_set_error("pool_solve: dataset %lld, option %lld: negative count %lld", (long long)i,
                               (long long)(j - opt_off[i]), (long long)counts[j]);
                return CATCHHIP_EINVAL;
            }
            if (!std::isfinite(losses[j])) {
                chip_set_error("pool_solve: dataset %lld, option %lld: the loss is not finite", (long long)i,
                               (long long)(j - opt_off[i]));
                return CATCHHIP_EINVAL;
            }
            lo = std::min(lo, counts[j]);
            hi = std::max(hi, counts[j]);
        }
        if (sum_min > std::numeric_limits<i64>::max() - lo || sum_max > std::numeric_limits<i64>::max() - hi) {
            chip_set_error("pool_solve: the counts add up to more than 2^63 - 1");
            return CATCHHIP_EINVAL;
        }
        sum_min += lo;
        sum_max += hi;
    }
    if (sum_min > budget) {
        chip_set_error("pool_solve: the budget of %lld probes cannot be met: the smallest feasible budget is %lld "
                       "(the sum of each dataset's smallest count)", (long long)budget, (long long)sum_min);
        return CATCHHIP_EINVAL;
    }
    if (D == 0) { *out_total = 0; *out_loss = 0.0; return 0; }
    // Cells above the sum of the largest counts are copies of that cell (every option fits at every step of the
    // walk from there, so values and ties are the same): a slack budget costs no more than a tight one.
    const i64 B = std::min(budget, sum_max);
    HIP_TRY(hipSetDevice(ctx->device));       // (the cache's limit is read from the current device on first use)
    const double table_bytes = (double)D * ((double)B + 1.0) * 2.0;
    if (B >= (i64)0xfffffffe || table_bytes + 16.0 * ((double)B + 1.0) > (double)chip_pool_soft_limit()) {
        chip_set_error("pool_solve: %lld datasets x %lld budget cells: the choice table (%.1f GB) is larger than the "
                       "device-memory cache may hold (%.1f GB)", (long long)D, (long long)B + 1, table_bytes / 1e9,
                       (double)chip_pool_soft_limit() / 1e9);
        return CATCHHIP_EINVAL;
    }
    const u32 ncell = (u32)(B + 1);
    const i64 nopt_all = opt_off[D];

    PoolScope pool_scope(ctx);
    hipStream_t s = ctx->stream;
    DevBuf<double> f_a, f_b, d_loss;
    DevBuf<u32> d_cnt;
    DevBuf<i64> d_off;
    DevBuf<uint16_t> d_choice;
    DevBuf<i32> d_out;
    DevBuf<unsigned long long> d_res;
    TRY(f_a.alloc(ncell));
    TRY(f_b.alloc(ncell));
    TRY(d_loss.alloc((size_t)nopt_all));
    TRY(d_cnt.alloc((size_t)nopt_all));
    TRY(d_off.alloc((size_t)D + 1));
    if (const int rc = d_choice.alloc((size_t)D * ncell)) {
        if (hipGetLastError() != hipErrorOutOfMemory) return rc;      // (the allocator's own message stands)
        // (the cache holds blocks of other contexts too: a table within the limit may still not fit beside them)
        chip_set_error("pool_solve: %lld datasets x %lld budget cells: no room for the choice table (%.1f GB) in the "
                       "device-memory cache", (long long)D, (long long)B + 1, table_bytes / 1e9);
        return CATCHHIP_EINVAL;
    }
    TRY(d_out.alloc((size_t)D));
    TRY(d_res.alloc(4));
    // staging: counts clamped to B + 1 as u32, then the results (i32[D] + 4 words)
    const size_t stage_bytes = std::max(sizeof(u32) * (size_t)nopt_all, sizeof(i32) * (size_t)D + 32);
    TRY(chip_pinned_reserve(ctx, stage_bytes));
    u32 *h_cnt = (u32 *)ctx->h_big;
    for (i64 j = 0; j < nopt_all; ++j) h_cnt[j] = (u32)std::min<i64>(counts[j], (i64)ncell);
    HIP_TRY(hipMemcpyAsync(d_cnt.p, h_cnt, sizeof(u32) * (size_t)nopt_all, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_loss.p, losses, sizeof(double) * (size_t)nopt_all, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_off.p, opt_off, sizeof(i64) * ((size_t)D + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(f_a.p, 0, sizeof(double) * (size_t)ncell, s));      // f_0 = 0.0
    PhaseTimer timer(ctx, PHASE_POOL);
    const dim3 grid((unsigned)div_up((i64)ncell, POOL_BLOCK)), blk(POOL_BLOCK);
    double *f_prev = f_a.p, *f_cur = f_b.p;
    for (i64 i = 0; i < D; ++i) {
        hipLaunchKernelGGL(pool_step_kernel, grid, blk, 0, s, (const double *)f_prev, f_cur,
                           d_choice.p + (size_t)i * ncell, (const u32 *)d_cnt.p + opt_off[i],
                           (const double *)d_loss.p + opt_off[i], (u32)(opt_off[i + 1] - opt_off[i]), ncell);
        std::swap(f_prev, f_cur);
    }
    hipLaunchKernelGGL(pool_trace_kernel, dim3(1), dim3(1), 0, s, (const uint16_t *)d_choice.p, (const u32 *)d_cnt.p,
                       (const i64 *)d_off.p, D, ncell, (const double *)f_prev, d_out.p, d_res.p);
    timer.launch(D + 1);
    timer.stop();
    HIP_TRY(hipGetLastError());
    // (the pinned area is free again: the copy of the counts was queued before the kernels that read them)
    i32 *h_out = (i32 *)ctx->h_big;
    unsigned long long *h_res = (unsigned long long *)((char *)ctx->h_big + ((sizeof(i32) * (size_t)D + 7) & ~(size_t)7));
    HIP_TRY(hipMemcpyAsync(h_out, d_out.p, sizeof(i32) * (size_t)D, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_res, d_res.p, sizeof(unsigned long long) * 2, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    timer.finish();
    memcpy(out_choice, h_out, sizeof(i32) * (size_t)D);
    *out_total = (i64)h_res[0];
    memcpy(out_loss, &h_res[1], sizeof(double));
    return 0;
}
