// Coverage analysis on the device beyond catchhip_rows_stats (scan.hip): where every probe was seen first
// (catchhip_rows_first_seen_per_set, at the end of this file) and the sliding-window depth of a row table
// (catchhip_rows_window_depth): the part of the analysis (catch/coverage_analysis.py:336-413) that walks every
// base of every genome.
//
//   1. chip_depth_diff     (depth.hip) span_mark_diff of every row: d[gs] += 1, d[ge] -= 1 over the global coordinates
//   2. chip_exclusive_scan_u32 in place: d[i] = sum of the differences before i, depth[pos] = d[pos + 1].  A row
//                          never leaves its universe, so the depth is 0 across every universe boundary and one scan
//                          over the whole coordinate space serves every span.
//   3. wd_tile_kernel      per tile of WD_TILE positions: exclusive prefix of (depth mod 2^16) inside the tile, written
//                          over d (a tile's sum is < 2^27, it fits the word), and the tile's sum as u64
//   4. wd_tilescan_kernel  exclusive prefix of the tile sums (u64), one workgroup
//   5. wd_window_kernel    one window per thread: P(end) - P(start) with P(x) = tile_off[x / WD_TILE] + d[x + 1]
//
// Everything is integer arithmetic; the host divides sum by count.
#include "rows_host.h"
#include "wave.h"

#include <algorithm>

#define WD_THREADS 256
#define WD_ITEMS 8
#define WD_TILE (WD_THREADS * WD_ITEMS)
#define WD_TILE_SHIFT 11
static_assert(WD_TILE == 1 << WD_TILE_SHIFT, "tile index is a shift");

// d[pos + 1] holds depth[pos] (mod 2^32) on entry and the sum of (depth mod 2^16) over [tile start, pos) on exit,
// for every pos <= total (the depth at pos == total counts as 0)
__global__ void __launch_bounds__(WD_THREADS)
wd_tile_kernel(u32 *__restrict__ d, u64 total, u64 *__restrict__ tile_sum) {
    __shared__ u32 lds[WD_THREADS / WAVE];
    const u64 base = (u64)blockIdx.x * WD_TILE + (u64)threadIdx.x * WD_ITEMS;
    u32 v[WD_ITEMS];
    u32 s = 0;
#pragma unroll
    for (int j = 0; j < WD_ITEMS; ++j) {
        v[j] = (base + j < total) ? (d[base + j + 1] & 0xffffu) : 0u;
        s += v[j];
    }
    // (block_excl_scan_u32 of wave.h written out below the wave scan: through that helper this kernel takes 34 VGPRs, not 33)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 inc = wave_incl_scan(s, lane);
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    u32 woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WD_THREADS / WAVE; ++w) {
        const u32 t = lds[w];
        if (w < wave) woff += t;
        tot += t;
    }
    u32 run = woff + inc - s;
#pragma unroll
    for (int j = 0; j < WD_ITEMS; ++j) {
        if (base + j <= total) d[base + j + 1] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

// exclusive prefix sum of n u64 values in place, one workgroup of 1024
__global__ void __launch_bounds__(1024)
wd_tilescan_kernel(u64 *__restrict__ t, u64 n) {
    __shared__ u64 lds[1024 / WAVE];
    __shared__ u64 s_carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (u64 base = 0; base < n; base += 1024) {
        const u64 i = base + threadIdx.x;
        const u64 v = i < n ? t[i] : 0;
        const u64 inc = wave_incl_scan(v, lane);
        if (lane == 63) lds[wave] = inc;
        __syncthreads();
        u64 woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 1024 / WAVE; ++w) {
            const u64 x = lds[w];
            if (w < wave) woff += x;
            tot += x;
        }
        const u64 carry = s_carry;
        if (i < n) t[i] = carry + woff + inc - v;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = carry + tot;
        __syncthreads();
    }
}

__device__ __forceinline__ u64 wd_prefix(const u32 *__restrict__ d, const u64 *__restrict__ tile_off, u64 x) {
    return tile_off[x >> WD_TILE_SHIFT] + d[x + 1];
}

// Window k of a span of n bases: [k * stride, k * stride + length), or when that passes the end the window
// numpy's counts[n - length : n] selects (:401-410): a negative start counts from the end and is clamped at 0.
__global__ void __launch_bounds__(256)
wd_window_kernel(const u32 *__restrict__ d, const u64 *__restrict__ tile_off, const u64 *__restrict__ win_off,
                 const u32 *__restrict__ span_lo, const u32 *__restrict__ span_n, u32 nspans, u64 nwin, u64 length,
                 u64 stride, u64 *__restrict__ sums, u32 *__restrict__ counts) {
    for (u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x; w < nwin; w += (u64)gridDim.x * blockDim.x) {
        // the last span that starts at or before w (empty spans share their successor's offset)
        u32 lo = 0, hi = nspans;
        while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (win_off[mid] <= w) lo = mid; else hi = mid; }
        const u64 n = span_n[lo], g0 = span_lo[lo];
        u64 a = (w - win_off[lo]) * stride, e = a + length;
        if (e > n) {
            e = n;
            a = n >= length ? n - length : (2 * n > length ? 2 * n - length : 0);
        }
        sums[w] = wd_prefix(d, tile_off, g0 + e) - wd_prefix(d, tile_off, g0 + a);
        counts[w] = (u32)(e - a);
    }
}

extern "C" int catchhip_rows_window_depth(catchhip_ctx *ctx, const catchhip_rows *R, const i64 *span_first, i64 nspans,
                                          i64 window_length, i64 window_stride, i64 *span_windows, u64 *sums,
                                          u32 *counts, i64 capacity) {
    ARG_CHECK(ctx && R && R->ctx == ctx && !R->deferred && nspans >= 0 && nspans < ((i64)1 << 31));
    ARG_CHECK(window_length >= 1 && window_stride >= 1);
    ARG_CHECK(nspans == 0 || (span_first && span_windows));
    ARG_CHECK((sums == nullptr) == (counts == nullptr));
    ARG_CHECK(R->total >= 0 && R->total < ((i64)1 << 32) - 4096);
    if (nspans == 0) return 0;
    if (span_first[0] < 0 || span_first[nspans] > R->ngenomes) {
        chip_set_error("rows_window_depth: the spans do not lie within the %d universes", (int)R->ngenomes);
        return CATCHHIP_EINVAL;
    }
    std::vector<u64> h_off((size_t)nspans + 1, 0);
    std::vector<u32> h_lo((size_t)nspans), h_n((size_t)nspans);
    for (i64 s = 0; s < nspans; ++s) {
        if (span_first[s + 1] < span_first[s] || span_first[s + 1] > R->ngenomes) {
            chip_set_error("rows_window_depth: span %lld ends before it starts or past the universes", (long long)s);
            return CATCHHIP_EINVAL;
        }
        const i64 g0 = R->h_genome_off[(size_t)span_first[s]], g1 = R->h_genome_off[(size_t)span_first[s + 1]];
        h_lo[s] = (u32)g0;
        h_n[s] = (u32)(g1 - g0);
        span_windows[s] = g1 > g0 ? (g1 - g0 - 1) / window_stride + 1 : 0;
        h_off[s + 1] = h_off[s] + (u64)span_windows[s];
    }
    if (!sums) return 0;   // the caller asked for the window counts only
    const u64 nwin = h_off[nspans];
    if ((u64)capacity < nwin) {
        chip_set_error("rows_window_depth: room for %lld windows, %llu needed", (long long)capacity,
                       (unsigned long long)nwin);
        return CATCHHIP_EINVAL;
    }
    if (nwin == 0) return 0;
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 total = (u64)R->total;
    const u64 ntiles = (total >> WD_TILE_SHIFT) + 1;   // position `total` itself has a prefix too
    DevBuf<u32> d, tmp, d_lo, d_n, d_counts;
    DevBuf<u64> tile_off, d_off, d_sums;
    TRY(d.alloc(total + 2));
    TRY(chip_exclusive_scan_reserve(tmp, (i64)total + 1));
    TRY(tile_off.alloc(ntiles));
    TRY(d_lo.alloc((size_t)nspans));
    TRY(d_n.alloc((size_t)nspans));
    TRY(d_off.alloc((size_t)nspans + 1));
    TRY(d_sums.alloc(nwin));
    TRY(d_counts.alloc(nwin));
    HIP_TRY(hipMemsetAsync(d.p, 0, sizeof(u32) * (total + 2), st));
    HIP_TRY(hipMemcpyAsync(d_lo.p, h_lo.data(), sizeof(u32) * (size_t)nspans, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_n.p, h_n.data(), sizeof(u32) * (size_t)nspans, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_off.p, h_off.data(), sizeof(u64) * ((size_t)nspans + 1), hipMemcpyHostToDevice, st));
    PhaseTimer tm(ctx, PHASE_ROWS);
    (void)chip_depth_diff(ctx, R, nullptr, 0u, d.p);
    TRY(chip_exclusive_scan_u32(ctx, d.p, d.p, (i64)total + 1, tmp));
    hipLaunchKernelGGL(wd_tile_kernel, dim3((unsigned)ntiles), dim3(WD_THREADS), 0, st, d.p, total, tile_off.p);
    hipLaunchKernelGGL(wd_tilescan_kernel, dim3(1), dim3(1024), 0, st, tile_off.p, ntiles);
    const u64 wblocks = std::min<u64>((nwin + 255) / 256, (u64)ctx->num_cus * 8);
    hipLaunchKernelGGL(wd_window_kernel, dim3((unsigned)wblocks), dim3(256), 0, st, (const u32 *)d.p,
                       (const u64 *)tile_off.p, (const u64 *)d_off.p, (const u32 *)d_lo.p, (const u32 *)d_n.p,
                       (u32)nspans, nwin, (u64)window_length, (u64)window_stride, d_sums.p, d_counts.p);
    tm.launch(7);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sums, d_sums.p, sizeof(u64) * nwin, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(counts, d_counts.p, sizeof(u32) * nwin, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    tm.finish();
    return 0;
}

// ------------------------------------------------------------------------
// where every set was seen first: rows are sorted by (set, universe, start), so the first row of a set lies in
// the first universe the set has rows in, and carries that (set, universe) group's first-discovery key
// ------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
rows_first_seen_kernel(const i32 *__restrict__ set_id, const i32 *__restrict__ univ,
                       const unsigned long long *__restrict__ first_key, u32 n, u32 num_sets,
                       i32 *__restrict__ out_univ, unsigned long long *__restrict__ out_key) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const i32 s = set_id[r];
    if ((r == 0 || set_id[r - 1] != s) && s >= 0 && (u32)s < num_sets) {
        out_univ[s] = univ[r];
        out_key[s] = first_key[r];
    }
}

extern "C" int catchhip_rows_first_seen_per_set(catchhip_ctx *ctx, const catchhip_rows *R, i64 num_sets,
                                                i32 *first_universe, u64 *first_key) {
    ARG_CHECK(ctx && R && R->ctx == ctx && !R->deferred && num_sets >= 0 && num_sets < ((i64)1 << 32));
    if (num_sets == 0) return 0;
    ARG_CHECK(first_universe && first_key);
    if (R->n && !R->first_key.p) {
        chip_set_error("rows_first_seen_per_set: these rows do not come from catchhip_cover_scan_first_seen");
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<i32> d_univ;
    DevBuf<unsigned long long> d_key;
    TRY(d_univ.alloc((size_t)num_sets));
    TRY(d_key.alloc((size_t)num_sets));
    HIP_TRY(hipMemsetAsync(d_univ.p, 0xff, sizeof(i32) * (size_t)num_sets, st));     // -1: no rows
    HIP_TRY(hipMemsetAsync(d_key.p, 0, sizeof(u64) * (size_t)num_sets, st));
    if (R->n)
        hipLaunchKernelGGL(rows_first_seen_kernel, dim3((unsigned)div_up(R->n, 256)), dim3(256), 0, st,
                           (const i32 *)R->set_id.p, (const i32 *)R->univ.p,
                           (const unsigned long long *)R->first_key.p, (u32)R->n, (u32)num_sets, d_univ.p, d_key.p);
    HIP_TRY(hipGetLastError());
    static_assert(sizeof(u64) == sizeof(unsigned long long), "64-bit keys");
    HIP_TRY(hipMemcpyAsync(first_universe, d_univ.p, sizeof(i32) * (size_t)num_sets, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(first_key, d_key.p, sizeof(u64) * (size_t)num_sets, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
