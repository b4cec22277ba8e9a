// Wavefront-level building blocks of the kernels: segment search, reductions, scans, DPP helpers.
// Device code only; gfx950, 64-lane wavefronts.  Unless a contract says otherwise, all 64 lanes of the wavefront
// must be active at the call (the shuffles and DPP moves read the neighbours' registers).
// Tested one by one through catchhip_selftest_wave / catchhip_selftest_find_segment (tests/test_primitives.py).
#pragma once
#include "internal.h"

// index s with off[s] <= x < off[s+1], empty segments skipped (off has n+1 entries, off[0] = 0, x < off[n]).
// Any lane on its own.
__device__ __forceinline__ u32 find_segment(const u32 *__restrict__ off, u32 n, u32 x) {
    u32 lo = 0, hi = n;  // answer in [lo, hi)
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    // skip empty segments: off[lo] <= x and we need x < off[lo+1]
    while (lo + 1 < n && off[lo + 1] <= x) ++lo;
    return lo;
}

// ---- reductions, __shfl_down form: LANE 0 holds the result, the other lanes hold partial values ----------------------
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, WAVE);
    return v;
}
template <typename T> __device__ __forceinline__ T wave_max(T v) {
    for (int d = 32; d > 0; d >>= 1) { const T o = __shfl_down(v, d, WAVE); v = o > v ? o : v; }
    return v;
}
// Several values (in place) through ONE loop, so that their shuffles interleave.
template <typename... T> __device__ __forceinline__ void wave_sum_n(T &...v) {
    for (int d = 32; d > 0; d >>= 1) ((v += __shfl_down(v, d, WAVE)), ...);
}
template <typename... T> __device__ __forceinline__ void wave_max_n(T &...v) {
    for (int d = 32; d > 0; d >>= 1) ((v = max(v, __shfl_down(v, d, WAVE))), ...);
}
// sum of s and maximum of m, one loop
template <typename S, typename M> __device__ __forceinline__ void wave_sum_max(S &s, M &m) {
    for (int d = 32; d > 0; d >>= 1) { s += __shfl_down(s, d, WAVE); m = max(m, __shfl_down(m, d, WAVE)); }
}

// ---- reductions, __shfl_xor form: EVERY lane holds the result ---------------------------------------------------------
template <typename T> __device__ __forceinline__ T wave_sum_all(T v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}
template <typename T> __device__ __forceinline__ T wave_max_all(T v) {
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, WAVE));
    return v;
}
template <typename... T> __device__ __forceinline__ void wave_sum_all_n(T &...v) {   // several values, one loop
    for (int d = 32; d > 0; d >>= 1) ((v += __shfl_xor(v, d, WAVE)), ...);
}
// sum over the aligned group of G lanes (a power of two), in every lane of the group
template <int G> __device__ __forceinline__ u32 group_sum(u32 v) {
#pragma unroll
    for (int d = 1; d < G; d <<= 1) v += __shfl_xor(v, d, WAVE);
    return v;
}

// ---- scans over the 64 lanes, __shfl_up form ----------------------------------------------------------------------------
// inclusive prefix sum (u32 or u64); lane = this thread's lane number; every lane holds its prefix
template <typename T> __device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const T t = __shfl_up(v, d, WAVE);
        if (lane >= d) v += t;
    }
    return v;
}
// exclusive prefix sum; *total = the wave's sum, in every lane
__device__ __forceinline__ u32 wave_excl_scan(u32 v, u32 *total) {
    const u32 incl = wave_incl_scan(v, (int)__lane_id());
    *total = __shfl(incl, 63);
    return incl - v;
}

// block-wide exclusive scan of one value per thread of a 256-thread workgroup (all threads call); returns the
// exclusive prefix, *block_total = sum over the block in every thread.  lds: 4 words, free again on return.
__device__ __forceinline__ u32 block_excl_scan_u32(u32 v, u32 *lds, u32 *block_total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 inc = wave_incl_scan(v, lane);
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    u32 woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 256 / WAVE; ++w) {
        u32 t = lds[w];
        if (w < wave) woff += t;
        tot += t;
    }
    __syncthreads();
    *block_total = tot;
    return woff + inc - v;
}

// ---- DPP helpers (register moves between lanes, no LDS permutes) ---------------------------------------------------
__device__ __forceinline__ u32 dpp_row_shl1(u32 v) {   // lane i <- lane i + 1 (inside a row of 16)
    return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, true);
}
__device__ __forceinline__ u32 quad_sum(u32 v) {       // sum over the 4 lanes of a quad, in every lane
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);    // quad_perm [1,0,3,2]
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);    // quad_perm [2,3,0,1]
    return v;
}
__device__ __forceinline__ u32 row8_sum(u32 v) {       // sum over the 8 lanes of a half row, in every lane
    v = quad_sum(v);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true);   // row_half_mirror
    return v;
}

// inclusive sum over the 64 lanes by DPP moves (no LDS permutes): Kogge-Stone inside the 16-lane rows (row_shr 1, 2, 4, 8,
// zero fill), then lane 15 of rows 0 / 2 added to rows 1 / 3 (row_bcast:15) and lane 31 to rows 2 and 3 (row_bcast:31)
__device__ __forceinline__ u32 wave_incl_scan_dpp(u32 v) {
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}

// inclusive sum over runs of equal keys in adjacent lanes; *tail = this lane ends its run.  Round 6: the wave's plain
// prefix sum by DPP moves minus its value just before the run's first lane -- one LDS permute instead of six (the six-step
// segmented scan through ds_bpermute was ~30 of the count launch's 190 VALU instructions per 64 rows).
__device__ __forceinline__ u32 wave_segsum(u32 v, u32 key, bool *tail) {
    const u32 lane = threadIdx.x & 63;
    const u32 kprev = (u32)__builtin_amdgcn_update_dpp((int)key, (int)key, 0x138, 0xf, 0xf, false);   // wave_shr:1 (lane 0: its own key, unused)
    const unsigned long long heads = __ballot(lane == 0 || kprev != key);
    // first lane of this lane's run: highest head at or below it
    const u32 start = 63u - (u32)__clzll(heads & (~0ull >> (63 - lane)));
    *tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    const u32 incl = wave_incl_scan_dpp(v);
    return incl - (u32)__shfl((int)(incl - v), (int)start, WAVE);      // minus the sum of the lanes before the run
}
