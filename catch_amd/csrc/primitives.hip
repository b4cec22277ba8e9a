// Device-wide primitives used by the cover-row builder and the near-duplicate
// filter: exclusive prefix sum and a stable LSD radix sort of (u64 key, u32
// value) pairs.  Hand-written for gfx950: 64-lane wavefronts, wave-level
// multi-split through __ballot, LDS for the per-workgroup digit tables.
#include "internal.h"
#include "spans.h"
#include "wave.h"

// ------------------------------------------------------------------------
// exclusive scan (u32): tile reduce -> recursive scan of tile sums -> tile scan
// ------------------------------------------------------------------------
#define SCAN_THREADS 256
#define SCAN_ITEMS 8
#define SCAN_TILE (SCAN_THREADS * SCAN_ITEMS)

static_assert(SCAN_THREADS == 256, "block_excl_scan_u32 scans a workgroup of 256");

__global__ void __launch_bounds__(SCAN_THREADS)
scan_tile_reduce(const u32 *__restrict__ in, u32 *__restrict__ tile_sums, i64 n) {
    __shared__ u32 lds[8];
    i64 base = (i64)blockIdx.x * SCAN_TILE + (i64)threadIdx.x * SCAN_ITEMS;
    u32 s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j)
        if (base + j < n) s += in[base + j];
    u32 tot;
    (void)block_excl_scan_u32(s, lds, &tot);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(SCAN_THREADS)
scan_tile_apply(const u32 *__restrict__ in, u32 *__restrict__ out,
                const u32 *__restrict__ tile_offs, i64 n) {
    __shared__ u32 lds[8];
    i64 base = (i64)blockIdx.x * SCAN_TILE + (i64)threadIdx.x * SCAN_ITEMS;
    u32 v[SCAN_ITEMS];
    u32 s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        v[j] = (base + j < n) ? in[base + j] : 0u;
        s += v[j];
    }
    u32 tot;
    u32 ex = block_excl_scan_u32(s, lds, &tot);
    u32 run = ex + (tile_offs ? tile_offs[blockIdx.x] : 0u);
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        if (base + j < n) out[base + j] = run;
        run += v[j];
    }
}

static int scan_rec(catchhip_ctx *ctx, const u32 *in, u32 *out, i64 n, u32 *tmp, i64 tmp_n) {
    if (n <= 0) return 0;
    i64 nt = div_up(n, SCAN_TILE);
    if (nt == 1) {
        hipLaunchKernelGGL(scan_tile_apply, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, in, out,
                           (const u32 *)nullptr, n);
        return 0;
    }
    if (tmp_n < nt) {
        chip_set_error("scan: scratch too small");
        return CATCHHIP_EINVAL;
    }
    hipLaunchKernelGGL(scan_tile_reduce, dim3((unsigned)nt), dim3(SCAN_THREADS), 0, ctx->stream, in,
                       tmp, n);
    TRY(scan_rec(ctx, tmp, tmp, nt, tmp + nt, tmp_n - nt));
    hipLaunchKernelGGL(scan_tile_apply, dim3((unsigned)nt), dim3(SCAN_THREADS), 0, ctx->stream, in,
                       out, (const u32 *)tmp, n);
    return 0;
}

int chip_exclusive_scan_reserve(DevBuf<u32> &tmp, i64 n) {
    i64 need = 0;
    for (i64 m = div_up(n, SCAN_TILE); m > 1; m = div_up(m, SCAN_TILE)) need += m;
    need += 4;
    return tmp.reserve((size_t)need);
}

int chip_exclusive_scan_u32(catchhip_ctx *ctx, const u32 *in, u32 *out, i64 n, DevBuf<u32> &tmp) {
    if (n <= 0) return 0;
    TRY(chip_exclusive_scan_reserve(tmp, n));
    TRY(scan_rec(ctx, in, out, n, tmp.p, (i64)tmp.n));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------
// LSD radix sort, 8-bit digits, stable.
// ------------------------------------------------------------------------
#define RS_THREADS 256
#define RS_ROUNDS 16
#define RS_TILE (RS_THREADS * RS_ROUNDS)

__global__ void __launch_bounds__(RS_THREADS)
radix_hist(const u64 *__restrict__ keys, i64 n, int shift, u32 *__restrict__ hist, u32 nblocks) {
    // (blockIdx.y = segment of a segmented sort: segments of n keys side by side, every segment sorted on its own)
    keys += (size_t)blockIdx.y * n;
    hist += (size_t)blockIdx.y * 256 * nblocks;
    __shared__ u32 h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    i64 base = (i64)blockIdx.x * RS_TILE;
#pragma unroll 4
    for (int r = 0; r < RS_ROUNDS; ++r) {
        i64 idx = base + (i64)r * RS_THREADS + threadIdx.x;
        if (idx < n) atomicAdd(&h[(u32)(keys[idx] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

// One pass of the scatter (round 4: tile-local sort first).  Rounds 1-3 ranked 256 keys per workgroup step and
// wrote every key straight to its place: ~1 key per digit and step, i.e. a lone 8-byte and a lone 4-byte write per
// key (134 M records of S4i's hit list: 2.6 ms per pass, ~1.2 TB/s of useful bytes).  Now a wavefront ranks its own
// 1,024 consecutive keys of the tile with wave-private digit counters (no workgroup barrier inside the 16 rounds),
// the tile is put in digit order in LDS, and the keys of one digit leave as one contiguous run.  Stable: a digit's
// keys keep the order (wavefront, round, lane) = their order in the input.
#define RS_WAVES (RS_THREADS / WAVE)
#define RS_PER_WAVE (RS_TILE / RS_WAVES)
__global__ void __launch_bounds__(RS_THREADS)
radix_scatter(const u64 *__restrict__ keys_in, const u32 *__restrict__ vals_in,
              u64 *__restrict__ keys_out, u32 *__restrict__ vals_out, i64 n, int shift,
              const u32 *__restrict__ hist_scanned, u32 nblocks) {
    __shared__ u64 s_key[RS_TILE];
    __shared__ u32 s_val[RS_TILE];
    __shared__ u32 wave_cnt[RS_WAVES][256];     // per wavefront: keys of each digit (then: its first slot in the tile order)
    __shared__ u32 dig_off[257];                // first tile slot of every digit
    __shared__ u32 gbase[256];                  // first output slot of every digit for this tile
    __shared__ u32 s_scan[RS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const i64 tile0 = (i64)blockIdx.x * RS_TILE;
    const u64 lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    {   // segment blockIdx.y: its keys, and its part of the histogram (scanned over ALL segments: minus the keys before it)
        const size_t seg = blockIdx.y;
        keys_in += seg * (size_t)n; vals_in += seg * (size_t)n; keys_out += seg * (size_t)n; vals_out += seg * (size_t)n;
        hist_scanned += seg * 256 * nblocks;
    }
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) wave_cnt[w][tid] = 0;
    gbase[tid] = hist_scanned[(size_t)tid * nblocks + blockIdx.x] - (u32)((size_t)blockIdx.y * (size_t)n);
    __syncthreads();
    u64 key[RS_ROUNDS];
    u32 val[RS_ROUNDS], rnk[RS_ROUNDS];       // rnk: rank among this wavefront's keys of the same digit
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; ++r) {
        const i64 idx = tile0 + (i64)wave * RS_PER_WAVE + (i64)r * WAVE + lane;
        const bool valid = idx < n;
        key[r] = valid ? keys_in[idx] : ~0ull;
        val[r] = valid ? vals_in[idx] : 0u;
        const u32 digit = (u32)(key[r] >> shift) & 255u;
        u64 peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const u64 bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        const u32 before = wave_cnt[wave][digit];          // (wave-private: LDS operations of one wavefront stay in order)
        rnk[r] = valid ? before + (u32)__popcll(peers & lt_mask) : 0xffffffffu;
        __builtin_amdgcn_wave_barrier();
        if (valid && (peers & lt_mask) == 0ull) wave_cnt[wave][digit] = before + (u32)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {   // thread tid = digit tid: its count in the tile, the wavefronts' shares of it, the exclusive scan over the digits
        u32 tot = 0;
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) { const u32 c = wave_cnt[w][tid]; wave_cnt[w][tid] = tot; tot += c; }
        u32 inc = wave_incl_scan(tot, lane);
        if (lane == 63) s_scan[wave] = inc;
        __syncthreads();
        u32 woff = 0;
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) if (w < wave) woff += s_scan[w];
        dig_off[tid] = woff + inc - tot;
        if (tid == 255) dig_off[256] = woff + inc;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_ROUNDS; ++r) {
        if (rnk[r] != 0xffffffffu) {
            const u32 digit = (u32)(key[r] >> shift) & 255u;
            const u32 q = dig_off[digit] + wave_cnt[wave][digit] + rnk[r];
            s_key[q] = key[r];
            s_val[q] = val[r];
        }
    }
    __syncthreads();
    const u32 ntile = dig_off[256];
    for (u32 q = tid; q < ntile; q += RS_THREADS) {
        const u64 k = s_key[q];
        const u32 digit = (u32)(k >> shift) & 255u;
        const u32 pos = gbase[digit] + (q - dig_off[digit]);
        keys_out[pos] = k;
        vals_out[pos] = s_val[q];
    }
}

int chip_radix_sort_pairs(catchhip_ctx *ctx, DevBuf<u64> &keys, DevBuf<u64> &keys_alt,
                          DevBuf<u32> &vals, DevBuf<u32> &vals_alt, i64 n, int key_bits, int first_bit) {
    if (n <= 1) return 0;
    if (n >= ((i64)1 << 32)) {
        chip_set_error("radix sort: n too large");
        return CATCHHIP_EINVAL;
    }
    TRY(keys_alt.reserve((size_t)n));
    TRY(vals_alt.reserve((size_t)n));
    u32 nblocks = (u32)div_up(n, RS_TILE);
    DevBuf<u32> hist, tmp;
    TRY(hist.alloc((size_t)256 * nblocks));
    int passes = (key_bits + 7) / 8;
    if (passes < 1) passes = 1;
    for (int p = 0; p < passes; ++p) {
        int shift = first_bit + 8 * p;
        hipLaunchKernelGGL(radix_hist, dim3(nblocks), dim3(RS_THREADS), 0, ctx->stream, keys.p, n,
                           shift, hist.p, nblocks);
        TRY(chip_exclusive_scan_u32(ctx, hist.p, hist.p, (i64)256 * nblocks, tmp));
        hipLaunchKernelGGL(radix_scatter, dim3(nblocks), dim3(RS_THREADS), 0, ctx->stream, keys.p,
                           vals.p, keys_alt.p, vals_alt.p, n, shift, hist.p, nblocks);
        keys.swap(keys_alt);
        vals.swap(vals_alt);
    }
    HIP_TRY(hipGetLastError());
    // scratch (hist/tmp) returns to the pool; reuse is ordered by the stream
    return 0;
}

// The same for `nseg` segments of n keys each, side by side in keys / vals (round 5: the 25 tables of a MinHash filter
// call in one go -- 350 sorts of ~10 launches per S5 step were 11,000 small launches queued behind other streams' kernels).
int chip_radix_sort_pairs_segments(catchhip_ctx *ctx, DevBuf<u64> &keys, DevBuf<u64> &keys_alt, DevBuf<u32> &vals,
                                   DevBuf<u32> &vals_alt, i64 n, i64 nseg, int key_bits, int first_bit) {
    if (n <= 1 || nseg <= 0) return 0;
    if (n * nseg >= ((i64)1 << 32) || nseg > 65535) {
        chip_set_error("radix sort: too many keys in all segments");
        return CATCHHIP_EINVAL;
    }
    TRY(keys_alt.reserve((size_t)(n * nseg)));
    TRY(vals_alt.reserve((size_t)(n * nseg)));
    const u32 nblocks = (u32)div_up(n, RS_TILE);
    DevBuf<u32> hist, tmp;
    TRY(hist.alloc((size_t)256 * nblocks * (size_t)nseg));
    int passes = (key_bits + 7) / 8;
    if (passes < 1) passes = 1;
    for (int p = 0; p < passes; ++p) {
        const int shift = first_bit + 8 * p;
        hipLaunchKernelGGL(radix_hist, dim3(nblocks, (unsigned)nseg), dim3(RS_THREADS), 0, ctx->stream, keys.p, n, shift, hist.p, nblocks);
        TRY(chip_exclusive_scan_u32(ctx, hist.p, hist.p, (i64)256 * nblocks * nseg, tmp));
        hipLaunchKernelGGL(radix_scatter, dim3(nblocks, (unsigned)nseg), dim3(RS_THREADS), 0, ctx->stream, keys.p, vals.p,
                           keys_alt.p, vals_alt.p, n, shift, hist.p, nblocks);
        keys.swap(keys_alt);
        vals.swap(vals_alt);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------
// Test entry points (tests/test_primitives.py): host data in, one call of the primitive (for the helpers of wave.h:
// one kernel that calls each of them), its result out.  No logic of their own beyond the copies.
// ------------------------------------------------------------------------
extern "C" int catchhip_selftest_scan_u32(catchhip_ctx *ctx, const u32 *in, i64 n, i32 in_place, u32 *out) {
    ARG_CHECK(ctx && n >= 0 && n < ((i64)1 << 32) && (n == 0 || (in && out)));
    PoolScope pool_scope(ctx);
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<u32> d_in, d_out, tmp;
    TRY(d_in.alloc((size_t)n));
    if (!in_place) TRY(d_out.alloc((size_t)n));
    HIP_TRY(hipMemcpyAsync(d_in.p, in, sizeof(u32) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    u32 *res = in_place ? d_in.p : d_out.p;
    TRY(chip_exclusive_scan_u32(ctx, d_in.p, res, n, tmp));
    HIP_TRY(hipMemcpyAsync(out, res, sizeof(u32) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int catchhip_selftest_sort_pairs(catchhip_ctx *ctx, u64 *keys, u32 *vals, i64 n, i64 nseg, i32 key_bits,
                                            i32 first_bit) {
    ARG_CHECK(ctx && n >= 0 && nseg >= 0 && nseg < ((i64)1 << 31) && n < ((i64)1 << 32));
    const i64 total = n * (nseg > 0 ? nseg : 1);
    ARG_CHECK(total < ((i64)1 << 32) && (total == 0 || (keys && vals)));
    PoolScope pool_scope(ctx);
    if (total == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<u64> d_keys, d_keys_alt;
    DevBuf<u32> d_vals, d_vals_alt;
    TRY(d_keys.alloc((size_t)total));
    TRY(d_vals.alloc((size_t)total));
    HIP_TRY(hipMemcpyAsync(d_keys.p, keys, sizeof(u64) * (size_t)total, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_vals.p, vals, sizeof(u32) * (size_t)total, hipMemcpyHostToDevice, ctx->stream));
    if (nseg == 0) TRY(chip_radix_sort_pairs(ctx, d_keys, d_keys_alt, d_vals, d_vals_alt, n, key_bits, first_bit));
    else TRY(chip_radix_sort_pairs_segments(ctx, d_keys, d_keys_alt, d_vals, d_vals_alt, n, nseg, key_bits, first_bit));
    HIP_TRY(hipMemcpyAsync(keys, d_keys.p, sizeof(u64) * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(vals, d_vals.p, sizeof(u32) * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// every helper of wave.h on one value per thread: out32[k * n + i] = result k of thread i, out64 likewise.  n is a
// multiple of 256, so every lane of every wavefront is at work.
#define WT_OUT32 10
#define WT_OUT64 2
__global__ void __launch_bounds__(256)
selftest_wave_kernel(const u32 *__restrict__ in, u32 n, u32 *__restrict__ out32, u64 *__restrict__ out64) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const u32 v = in[i];
    const u64 v64 = ((u64)(v & 0xffffu) << 32) | v;
    u32 total;
    const u32 excl = wave_excl_scan(v, &total);
    const u32 r[WT_OUT32] = {wave_sum(v), wave_max(v), wave_sum_all(v), wave_max_all(v), wave_incl_scan(v, lane), excl, total,
                             wave_incl_scan_dpp(v), quad_sum(v), row8_sum(v)};
#pragma unroll
    for (int k = 0; k < WT_OUT32; ++k) out32[(size_t)k * n + i] = r[k];
    out64[i] = wave_max(v64);
    out64[(size_t)n + i] = wave_incl_scan(v64, lane);
}

__global__ void __launch_bounds__(256)
selftest_find_segment_kernel(const u32 *__restrict__ off, u32 n, const u32 *__restrict__ x, u32 nx, u32 *__restrict__ out) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i < nx) out[i] = find_segment(off, n, x[i]);
}

extern "C" int catchhip_selftest_wave(catchhip_ctx *ctx, const u32 *in, i64 n, u32 *out32, u64 *out64) {
    ARG_CHECK(ctx && in && out32 && out64 && n > 0 && n % 256 == 0 && n <= ((i64)1 << 24));
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<u32> d_in, d_out32;
    DevBuf<u64> d_out64;
    TRY(d_in.alloc((size_t)n));
    TRY(d_out32.alloc((size_t)n * WT_OUT32));
    TRY(d_out64.alloc((size_t)n * WT_OUT64));
    HIP_TRY(hipMemcpyAsync(d_in.p, in, sizeof(u32) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(selftest_wave_kernel, dim3((unsigned)(n / 256)), dim3(256), 0, ctx->stream, (const u32 *)d_in.p,
                       (u32)n, d_out32.p, d_out64.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out32, d_out32.p, sizeof(u32) * (size_t)n * WT_OUT32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out64, d_out64.p, sizeof(u64) * (size_t)n * WT_OUT64, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int catchhip_selftest_find_segment(catchhip_ctx *ctx, const u32 *off, i64 n, const u32 *x, i64 nx, u32 *out) {
    ARG_CHECK(ctx && off && x && out && n >= 1 && n < ((i64)1 << 31) && nx >= 1 && nx < ((i64)1 << 31));
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<u32> d_off, d_x, d_out;
    TRY(d_off.alloc((size_t)n + 1));
    TRY(d_x.alloc((size_t)nx));
    TRY(d_out.alloc((size_t)nx));
    HIP_TRY(hipMemcpyAsync(d_off.p, off, sizeof(u32) * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_x.p, x, sizeof(u32) * (size_t)nx, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(selftest_find_segment_kernel, dim3((unsigned)div_up(nx, 256)), dim3(256), 0, ctx->stream,
                       (const u32 *)d_off.p, (u32)n, (const u32 *)d_x.p, (u32)nx, d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out.p, sizeof(u32) * (size_t)nx, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// every helper of spans.h on one interval [a[i], b[i]) per thread, over the caller's bitmap: out32[k * n + i] = first
// word, words, span_popc, span_all_set; out64[k * n + i] = m0, m1, span_in_word for word `view` (0: they do not overlap)
__global__ void __launch_bounds__(256)
selftest_spans_kernel(const unsigned long long *__restrict__ bm, const u32 *__restrict__ a, const u32 *__restrict__ b, u32 n,
                      u32 view, u32 *__restrict__ out32, u64 *__restrict__ out64) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Span sp = span_of(a[i], b[i]);
    const u64 base = (u64)view << 6;
    const u32 r[4] = {sp.w0, sp.nw, span_popc(bm, a[i], b[i]), span_all_set(bm, a[i], b[i]) ? 1u : 0u};
    for (int k = 0; k < 4; ++k) out32[(size_t)k * n + i] = r[k];
    out64[i] = sp.m0;
    out64[(size_t)n + i] = sp.m1;
    out64[2 * (size_t)n + i] = (a[i] < base + 64 && b[i] > base) ? span_in_word(base, a[i], b[i]) : 0ull;
}
// all intervals into one zeroed bitmap and one zeroed difference array
__global__ void __launch_bounds__(256)
selftest_spans_paint_kernel(const u32 *__restrict__ a, const u32 *__restrict__ b, u32 n, unsigned long long *__restrict__ bm,
                            u32 *__restrict__ d) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    span_paint(bm, a[i], b[i]);
    span_mark_diff(d, a[i], b[i]);
}

extern "C" int catchhip_selftest_spans(catchhip_ctx *ctx, const u64 *bm, i64 nwords, const u32 *a, const u32 *b, i64 n,
                                       u32 view, u32 *out32, u64 *out64, u64 *painted, u32 *diff) {
    ARG_CHECK(ctx && bm && a && b && out32 && out64 && painted && diff);
    ARG_CHECK(nwords >= 1 && nwords <= ((i64)1 << 20) && n >= 1 && n <= ((i64)1 << 20) && (i64)view < nwords);
    for (i64 i = 0; i < n; ++i) ARG_CHECK(a[i] < b[i] && (i64)b[i] <= 64 * nwords);      // (the kernels index by them)
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t nw = (size_t)nwords, nd = 64 * nw + 1, ni = (size_t)n;
    DevBuf<unsigned long long> d_bm, d_painted;
    DevBuf<u32> d_ab, d_out32, d_diff;                       // (a, then b)
    DevBuf<u64> d_out64;
    TRY(d_bm.alloc(nw));
    TRY(d_painted.alloc(nw));
    TRY(d_ab.alloc(2 * ni));
    TRY(d_out32.alloc(4 * ni));
    TRY(d_out64.alloc(3 * ni));
    TRY(d_diff.alloc(nd));
    HIP_TRY(hipMemcpyAsync(d_bm.p, bm, sizeof(u64) * nw, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_ab.p, a, sizeof(u32) * ni, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_ab.p + ni, b, sizeof(u32) * ni, hipMemcpyHostToDevice, s));
    const u32 *d_a = d_ab.p, *d_b = d_ab.p + ni;
    HIP_TRY(hipMemsetAsync(d_painted.p, 0, sizeof(u64) * nw, s));
    HIP_TRY(hipMemsetAsync(d_diff.p, 0, sizeof(u32) * nd, s));
    const dim3 grid((unsigned)div_up(n, 256)), blk(256);
    hipLaunchKernelGGL(selftest_spans_kernel, grid, blk, 0, s, (const unsigned long long *)d_bm.p, d_a, d_b, (u32)n, view,
                       d_out32.p, d_out64.p);
    hipLaunchKernelGGL(selftest_spans_paint_kernel, grid, blk, 0, s, d_a, d_b, (u32)n, d_painted.p, d_diff.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out32, d_out32.p, sizeof(u32) * 4 * ni, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out64, d_out64.p, sizeof(u64) * 3 * ni, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(painted, d_painted.p, sizeof(u64) * nw, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(diff, d_diff.p, sizeof(u32) * nd, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}
