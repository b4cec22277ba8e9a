// design_naively's two filters: the redundancy graph of a probe list, the naive
// pass over it and the rows of its dominating-set cover
// (catchhip_redundancy_graph / _naive / _rows).
//
// The reference evaluates a pairwise predicate over all n (n - 1) / 2 pairs in
// Python (catch/filter/naive_redundant_filter.py:46-77, catch/filter/
// dominating_set_filter.py:62-91) and therefore puts a randomised k-mer
// heuristic in front of it; here the exact predicate runs for every pair.
//
// Every probe is packed into three bit-planes (two code bits and an N bit) of W
// 64-bit words, W in {1, 2, 4} by the longest probe.  A block owns a 64 x 64
// tile of the upper triangle of the pair matrix and stages both sides' planes
// in LDS; a wave takes 16 rows of the tile, one column per lane, so the row's
// planes are a broadcast read and the column's a conflict-free one.  Per
// diagonal d (probe a shifted by d against probe b) the shifted operand is a
// funnel shift of two LDS words per plane, the mismatch mask is
//     X = ((a0 ^ b0) | (a1 ^ b1) | (aN ^ bN)) & overlap
// -- plain character inequality, N equals N -- and
//   kind 0 (redundant_shift_and_mismatch_count): popcount(X) <= mismatch_thres
//          for some |d| <= shift; an empty overlap has no mismatch;
//   kind 1 (redundant_longest_common_substring, k_lcf >= lcf_thres): on a
//          diagonal of overlap O >= lcf_thres some window of exactly lcf_thres
//          positions holds <= mismatches set bits.  popcount(X) <= mismatches
//          accepts, popcount(X) > mismatches + (O - lcf_thres) rejects (every
//          window leaves out at most O - lcf_thres positions); otherwise two
//          cursors walk the set bits mismatches + 1 apart and test the gaps.
// The verdicts of a wave's row are one ballot = one word of the adjacency bitmap
// (row i, word tile_j); the transposed bits are gathered per lane and OR-ed into
// (row j, word tile_i).  Degrees are popcounts, one block scans them into 64-bit
// offsets and a wave per row writes its neighbours out of the bitmap, ascending
// without a sort.
#include <algorithm>

#include "redgraph.h"
#include "rows_host.h"
#include "wave.h"

#define RN_ROUNDS 8            // frontier rounds per read-back of the naive pass
#define RN_FEW 64              // a round that decides fewer vertices hands over to the one-workgroup walk
#define RN_BLOCK 1024

// one 64-base word of a probe's three planes: A = 0, C = 1, G = 2, T = 3, N = code 0 with the N bit
__host__ __device__ static inline void rg_pack_word(const u8 *chars, u32 len, int w, u64 *c0, u64 *c1, u64 *cn) {
    u64 x0 = 0, x1 = 0, xn = 0;
    const u32 lo = (u32)w * 64, hi = len < lo + 64 ? len : lo + 64;
    for (u32 i = lo; i < hi; ++i) {
        const u8 ch = chars[i];
        const u32 code = ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 0u;
        x0 |= (u64)(code & 1) << (i - lo);
        x1 |= (u64)(code >> 1) << (i - lo);
        xn |= (u64)(ch == 'N') << (i - lo);
    }
    *c0 = x0; *c1 = x1; *cn = xn;
}

// planes[(plane * W + w) * npad + probe]; probes beyond n and bits beyond a probe's length stay zero
__global__ void rg_pack_kernel(const u8 *__restrict__ bytes, const i64 *__restrict__ off, u32 n, u32 npad, int W,
                               u64 *__restrict__ planes, u32 *__restrict__ lens) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const i64 a = off[p];
    const u32 len = (u32)(off[p + 1] - a);
    lens[p] = len;
    for (int w = 0; w < W; ++w) {
        u64 c0, c1, cn;
        rg_pack_word(bytes + a, len, w, &c0, &c1, &cn);
        planes[((size_t)(0 * W + w)) * npad + p] = c0;
        planes[((size_t)(1 * W + w)) * npad + p] = c1;
        planes[((size_t)(2 * W + w)) * npad + p] = cn;
    }
}

// the lowest set bit of X at a position >= from (0 <= from <= 64 W); 64 W when there is none
template <int W> __host__ __device__ static inline int rg_next_set(const u64 (&X)[W], int from) {
    int res = 64 * W;
#pragma unroll
    for (int w = W - 1; w >= 0; --w) {
        const int rel = from - 64 * w;
        const u64 mk = rel <= 0 ? ~0ull : (rel >= 64 ? 0ull : (~0ull << rel));
        const u64 v = X[w] & mk;
        if (v) res = 64 * w + __builtin_ffsll((long long)v) - 1;
    }
    return res;
}

// The predicate for one pair.  a / b point at word 0 of plane 0 of the two probes in a tile's layout
// [plane][2 W words][RG_TILE probes] (words W .. 2 W - 1 zero: a shifted read never leaves the array); la / lb are
// their lengths.  Diagonal d compares a[p + d] with b[p] (d >= 0) or a[p] with b[p - d] (d < 0) over the overlap O.
template <int W, int KIND>
__host__ __device__ static inline bool rg_pair(const u64 *a, const u64 *b, int la, int lb, i32 p0, i32 p1) {
    // diagonals looked at: kind 0 |d| <= shift (beyond 64 W every overlap is empty); kind 1 the ones whose
    // overlap can reach lcf_thres
    const int dmax = KIND == 0 ? (p0 < 64 * W ? p0 : 64 * W) : 64 * W - p1;
    for (int d = -dmax; d <= dmax; ++d) {
        const int i0 = d > 0 ? d : 0, j0 = d < 0 ? -d : 0;
        const int O = la - i0 < lb - j0 ? la - i0 : lb - j0;
        if (KIND == 1 && O < p1) continue;
        // the shifted operand: probe a for d >= 0, probe b for d < 0
        const int s = i0 + j0 < 64 * W - 1 ? i0 + j0 : 64 * W - 1;
        const int ws = s >> 6, bs = s & 63;
        const u64 *sh = d >= 0 ? a : b, *un = d >= 0 ? b : a;
        u64 X[W];
        int pc = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            u64 x = 0;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                const u64 lo = sh[(size_t)(pl * 2 * W + w + ws) * RG_TILE], hi = sh[(size_t)(pl * 2 * W + w + ws + 1) * RG_TILE];
                const u64 shifted = (lo >> bs) | ((hi << 1) << (63 - bs));
                x |= shifted ^ un[(size_t)(pl * 2 * W + w) * RG_TILE];
            }
            const int rem = O - 64 * w;
            x &= rem <= 0 ? 0ull : (rem >= 64 ? ~0ull : ((1ull << rem) - 1));
            X[w] = x;
            pc += __builtin_popcountll(x);
        }
        if (KIND == 0) {
            if (pc <= p1) return true;
        } else if (pc <= p0) {
            return true;
        } else if (pc <= p0 + (O - p1)) {
            // gaps between set bits p0 + 1 apart, the ends of the overlap standing in as set bits
            int trail = -1, lead = -1;
            for (int k = 0; k <= p0; ++k) lead = rg_next_set<W>(X, lead + 1);
            for (;;) {
                if (lead > O) lead = O;
                if (lead - trail - 1 >= p1) return true;
                if (lead >= O) break;
                trail = rg_next_set<W>(X, trail + 1);
                lead = rg_next_set<W>(X, lead + 1);
            }
        }
    }
    return false;
}

// One 64 x 64 tile of pairs (rows ti * 64 .., columns tj * 64 .., ti <= tj); pair (gi, gj) counts when gi < gj < n.
template <int W, int KIND>
__global__ void __launch_bounds__(RG_BLOCK)
rg_pairs_kernel(const u64 *__restrict__ planes, const u32 *__restrict__ lens, u32 n, u32 npad, i32 p0, i32 p1,
                unsigned long long *__restrict__ bitmap, u32 rowwords) {
    const u32 ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    __shared__ u64 s_pl[2][3][2 * W][RG_TILE];
    __shared__ u32 s_len[2][RG_TILE];
    for (u32 t = threadIdx.x; t < 2 * 3 * 2 * W * RG_TILE; t += RG_BLOCK) {
        const u32 pr = t % RG_TILE, w = (t / RG_TILE) % (2 * W), pl = (t / (RG_TILE * 2 * W)) % 3, side = t / (RG_TILE * 2 * W * 3);
        const u32 g = (side ? tj : ti) * RG_TILE + pr;      // < npad
        s_pl[side][pl][w][pr] = w < (u32)W ? planes[((size_t)(pl * W + w)) * npad + g] : 0ull;
    }
    if (threadIdx.x < 2 * RG_TILE) {
        const u32 side = threadIdx.x / RG_TILE, pr = threadIdx.x % RG_TILE;
        s_len[side][pr] = lens[(side ? tj : ti) * RG_TILE + pr];
    }
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 gj = tj * RG_TILE + lane;
    const int lb = (int)s_len[1][lane];
    u64 colmask = 0;
    for (u32 r = wave; r < RG_TILE; r += RG_BLOCK / 64) {
        const u32 gi = ti * RG_TILE + r;
        const bool valid = gi < gj && gj < n;
        const bool hit = valid && rg_pair<W, KIND>(&s_pl[0][0][0][r], &s_pl[1][0][0][lane], (int)s_len[0][r], lb, p0, p1);
        const unsigned long long bal = __ballot(hit);
        if (bal && lane == 0) atomicOr(&bitmap[(size_t)gi * rowwords + tj], bal);
        colmask |= (u64)hit << r;
    }
    if (colmask) atomicOr(&bitmap[(size_t)gj * rowwords + ti], (unsigned long long)colmask);
}

// degrees: one wave per row
__global__ void __launch_bounds__(256)
rg_degree_kernel(const unsigned long long *__restrict__ bitmap, u32 n, u32 rowwords, u32 *__restrict__ deg) {
    const u32 row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    u32 c = 0;
    for (u32 w = lane; w < rowwords; w += 64) c += (u32)__popcll(bitmap[(size_t)row * rowwords + w]);
    c = wave_sum_all(c);
    if (lane == 0) deg[row] = c;
}

// ptr[0 .. n] = exclusive scan of deg in 64 bits; one block, a contiguous run of values per thread
__global__ void __launch_bounds__(RN_BLOCK)
rg_scan_kernel(const u32 *__restrict__ deg, u32 n, i64 *__restrict__ ptr) {
    __shared__ i64 s_sum[RN_BLOCK];
    const u32 per = (n + RN_BLOCK - 1) / RN_BLOCK;
    const u32 a = min(n, threadIdx.x * per), b = min(n, a + per);
    i64 sum = 0;
    for (u32 i = a; i < b; ++i) sum += deg[i];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (u32 o = 1; o < RN_BLOCK; o <<= 1) {
        const i64 v = threadIdx.x >= o ? s_sum[threadIdx.x - o] : 0;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    i64 run = s_sum[threadIdx.x] - sum;
    for (u32 i = a; i < b; ++i) { ptr[i] = run; run += deg[i]; }
    if (threadIdx.x == RN_BLOCK - 1) ptr[n] = s_sum[RN_BLOCK - 1];
}

// neighbours of a row out of its bitmap words, ascending: one wave per row
__global__ void __launch_bounds__(256)
rg_fill_kernel(const unsigned long long *__restrict__ bitmap, u32 n, u32 rowwords, const i64 *__restrict__ ptr,
               u32 *__restrict__ idx) {
    const u32 row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    i64 base = ptr[row];
    for (u32 w0 = 0; w0 < rowwords; w0 += 64) {
        const u32 w = w0 + lane;
        u64 word = w < rowwords ? bitmap[(size_t)row * rowwords + w] : 0ull;
        const u32 c = (u32)__popcll(word);
        const u32 incl = wave_incl_scan(c, (int)lane);
        i64 at = base + (incl - c);
        while (word) {
            const int b = __ffsll((long long)word) - 1;
            idx[at++] = w * 64 + (u32)b;
            word &= word - 1;
        }
        base += __shfl(incl, 63);
    }
}

// ---- naive pass: the lexicographically first maximal independent set ----------------------------------------------
// state: 0 undecided, 1 kept, 2 dropped.  A vertex is dropped once a smaller neighbour is kept and kept once all
// smaller neighbours are dropped; a state read while its owner decides is at worst still 0, which decides nothing.
__global__ void __launch_bounds__(256)
rn_round_kernel(const i64 *__restrict__ ptr, const u32 *__restrict__ idx, u32 n, u8 *state, u32 *__restrict__ left) {
    const u32 v = blockIdx.x * 256 + threadIdx.x;
    bool undecided = false;
    if (v < n && state[v] == 0) {
        u8 res = 0;
        bool all_dropped = true;
        const i64 end = ptr[v + 1];
        for (i64 e = ptr[v]; e < end; ++e) {
            const u32 u = idx[e];
            if (u >= v) break;
            const u8 s = state[u];
            if (s == 1) { res = 2; break; }
            if (s == 0) all_dropped = false;
        }
        if (!res && all_dropped) res = 1;
        if (res) state[v] = res;
        else undecided = true;
    }
    const unsigned long long bal = __ballot(undecided);
    if (bal && (threadIdx.x & 63) == 0) atomicAdd(left, (u32)__popcll(bal));
}

__device__ static inline u8 rn_load(const u8 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The rest in ONE workgroup, chunks of RN_BLOCK vertices in order: everything below a chunk is decided, the chunk's
// own states live in LDS and it iterates until none of them is undecided (its smallest undecided vertex is decided
// in every iteration).  A cursor per vertex skips the neighbours already seen dropped.
__global__ void __launch_bounds__(RN_BLOCK)
rn_finish_kernel(const i64 *__restrict__ ptr, const u32 *__restrict__ idx, u32 n, u8 *state) {
    __shared__ u8 s_st[RN_BLOCK];
    __shared__ u32 s_left;
    for (u32 base = 0; base < n; base += RN_BLOCK) {
        const u32 v = base + threadIdx.x;
        const bool live = v < n;
        u8 st = live ? state[v] : (u8)2;
        const bool mine = live && st == 0;
        i64 e = live ? ptr[v] : 0;
        const i64 end = live ? ptr[v + 1] : 0;
        s_st[threadIdx.x] = st;
        for (;;) {
            if (threadIdx.x == 0) s_left = 0;
            __syncthreads();
            if (live && st == 0) {
                u8 res = 1;                       // kept unless a smaller neighbour says otherwise
                while (e < end) {
                    const u32 u = idx[e];
                    if (u >= v) break;
                    const u8 s = u >= base ? s_st[u - base] : rn_load(state + u);
                    if (s == 2) { ++e; continue; }
                    res = s == 1 ? (u8)2 : (u8)0;
                    break;
                }
                if (res) st = res;
                else atomicAdd(&s_left, 1u);
            }
            __syncthreads();
            s_st[threadIdx.x] = st;
            const u32 left = s_left;
            __syncthreads();
            if (!left) break;
        }
        if (mine) __hip_atomic_store(state + v, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
    }
}

__global__ void rn_keep_kernel(const u8 *__restrict__ state, u32 n, u8 *__restrict__ keep) {
    const u32 v = blockIdx.x * 256 + threadIdx.x;
    if (v < n) keep[v] = state[v] == 1;
}

// ---- dominating set: the rows of the sets S_i = {i} + N(i) ---------------------------------------------------------
// Element u sits at coordinate 2 u, so the rows [2 u, 2 u + 1) of a set are disjoint and never touch.  Set i owns the
// slots ptr[i] + i .. ptr[i + 1] + i: its neighbours in order with i itself merged in.
__global__ void __launch_bounds__(256)
rr_rows_kernel(const i64 *__restrict__ ptr, const u32 *__restrict__ idx, u32 n, i32 *__restrict__ set_id,
               i32 *__restrict__ univ, u32 *__restrict__ gs, u32 *__restrict__ ge) {
    const u32 i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const i64 p = ptr[i];
    const i64 deg = ptr[i + 1] - p;
    for (i64 k = lane; k <= deg; k += 64) {
        u32 elem;
        if (k < deg && idx[p + k] < i) elem = idx[p + k];
        else {
            const u32 prev = k > 0 ? idx[p + k - 1] : 0u;
            elem = (k == 0 || prev < i) ? i : prev;
        }
        const i64 at = p + i + k;
        set_id[at] = (i32)i;
        univ[at] = 0;
        gs[at] = 2 * elem;
        ge[at] = 2 * elem + 1;
    }
}

template <int W>
static void rg_launch_pairs(hipStream_t s, dim3 grid, i32 kind, const u64 *planes, const u32 *lens, u32 n, u32 npad, i32 p0,
                            i32 p1, unsigned long long *bitmap, u32 rowwords) {
    if (kind == 0)
        hipLaunchKernelGGL((rg_pairs_kernel<W, 0>), grid, dim3(RG_BLOCK), 0, s, planes, lens, n, npad, p0, p1, bitmap, rowwords);
    else
        hipLaunchKernelGGL((rg_pairs_kernel<W, 1>), grid, dim3(RG_BLOCK), 0, s, planes, lens, n, npad, p0, p1, bitmap, rowwords);
}

extern "C" int catchhip_redundancy_graph(catchhip_ctx *ctx, const u8 *bytes, const i64 *off, i64 n, i32 kind, i32 p0,
                                         i32 p1, catchhip_redgraph **out, i64 *nedges) {
    ARG_CHECK(ctx && out && off && n >= 0 && (kind == 0 || kind == 1) && (n == 0 || bytes));
    *out = nullptr;
    if (p0 < 0) {
        chip_set_error("redundancy_graph: %s must not be negative (%d)", kind == 0 ? "shift" : "mismatches", p0);
        return CATCHHIP_EINVAL;
    }
    if (kind == 1 && p1 <= 0) {
        chip_set_error("redundancy_graph: lcf_thres %d makes every pair redundant; the caller answers that itself", p1);
        return CATCHHIP_EINVAL;
    }
    i64 maxlen = 0;
    for (i64 i = 0; i < n; ++i) {
        const i64 len = off[i + 1] - off[i];
        if (len < 0) { chip_set_error("redundancy_graph: offsets of probe %lld decrease", (long long)i); return CATCHHIP_EINVAL; }
        if (len > RG_MAXLEN) {
            chip_set_error("redundancy_graph: probe %lld has %lld bases; the kernel compares at most %d", (long long)i,
                           (long long)len, RG_MAXLEN);
            return CATCHHIP_EINVAL;
        }
        maxlen = std::max(maxlen, len);
        for (i64 j = off[i]; j < off[i + 1]; ++j) {
            const u8 c = bytes[j];
            if (c != 'A' && c != 'C' && c != 'G' && c != 'T' && c != 'N') {
                chip_set_error("redundancy_graph: probe %lld holds a letter outside ACGTN (byte %u)", (long long)i, (unsigned)c);
                return CATCHHIP_EINVAL;
            }
        }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const i64 tiles = div_up(std::max<i64>(n, 1), RG_TILE);
    const i64 npad = tiles * RG_TILE;
    const double bitmap_bytes = (double)n * (double)tiles * 8.0;
    if (tiles > 65535 || bitmap_bytes > 0.5 * (double)chip_pool_soft_limit()) {
        chip_set_error("redundancy_graph: %lld probes: the adjacency bitmap (%.1f GB) is larger than half of what the "
                       "device-memory cache may hold (%.1f GB)", (long long)n, bitmap_bytes / 1e9,
                       (double)chip_pool_soft_limit() / 1e9);
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    hipStream_t s = ctx->stream;
    std::unique_ptr<catchhip_redgraph> G(new catchhip_redgraph());
    G->ctx = ctx;
    G->n = n;
    TRY(G->ptr.alloc((size_t)n + 1));
    if (n == 0) {   // the empty graph
        HIP_TRY(hipMemsetAsync(G->ptr.p, 0, sizeof(i64), s));
        HIP_TRY(hipStreamSynchronize(s));
        TRY(G->idx.alloc(1));
        if (nedges) *nedges = 0;
        *out = G.release();
        return 0;
    }
    const int W = maxlen <= 64 ? 1 : maxlen <= 128 ? 2 : 4;
    const i64 total = off[n] - off[0];
    DevBuf<u8> d_bytes;
    DevBuf<i64> d_off;
    DevBuf<u64> planes;
    DevBuf<u32> lens, deg;
    DevBuf<unsigned long long> bitmap;
    TRY(d_bytes.alloc((size_t)total + 1));
    TRY(d_off.alloc((size_t)n + 1));
    TRY(planes.alloc((size_t)3 * W * npad));
    TRY(lens.alloc((size_t)npad));
    TRY(deg.alloc((size_t)n));
    TRY(bitmap.alloc((size_t)n * tiles));
    // (offsets relative to the first byte handed over)
    std::vector<i64> rel((size_t)n + 1);
    for (i64 i = 0; i <= n; ++i) rel[i] = off[i] - off[0];
    if (total) HIP_TRY(hipMemcpyAsync(d_bytes.p, bytes + off[0], (size_t)total, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_off.p, rel.data(), sizeof(i64) * ((size_t)n + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(planes.p, 0, sizeof(u64) * (size_t)3 * W * npad, s));
    HIP_TRY(hipMemsetAsync(lens.p, 0, sizeof(u32) * (size_t)npad, s));
    HIP_TRY(hipMemsetAsync(bitmap.p, 0, sizeof(u64) * (size_t)n * tiles, s));
    PhaseTimer timer(ctx, PHASE_NDF);
    hipLaunchKernelGGL(rg_pack_kernel, dim3((unsigned)div_up(n, 256)), dim3(256), 0, s, (const u8 *)d_bytes.p,
                       (const i64 *)d_off.p, (u32)n, (u32)npad, W, planes.p, lens.p);
    const dim3 grid((unsigned)tiles, (unsigned)tiles);
    if (W == 1) rg_launch_pairs<1>(s, grid, kind, planes.p, lens.p, (u32)n, (u32)npad, p0, p1, bitmap.p, (u32)tiles);
    else if (W == 2) rg_launch_pairs<2>(s, grid, kind, planes.p, lens.p, (u32)n, (u32)npad, p0, p1, bitmap.p, (u32)tiles);
    else rg_launch_pairs<4>(s, grid, kind, planes.p, lens.p, (u32)n, (u32)npad, p0, p1, bitmap.p, (u32)tiles);
    timer.launch(2);
    TRY(chip_redgraph_from_bitmap(ctx, timer, bitmap.p, tiles, deg.p, G.get()));
    if (nedges) *nedges = G->nedges;
    *out = G.release();
    return 0;
}

int chip_redgraph_from_bitmap(catchhip_ctx *ctx, PhaseTimer &timer, const unsigned long long *bitmap, i64 tiles, u32 *deg,
                              catchhip_redgraph *G) {
    hipStream_t s = ctx->stream;
    const i64 n = G->n;
    hipLaunchKernelGGL(rg_degree_kernel, dim3((unsigned)div_up(n, 4)), dim3(256), 0, s, bitmap, (u32)n, (u32)tiles, deg);
    hipLaunchKernelGGL(rg_scan_kernel, dim3(1), dim3(RN_BLOCK), 0, s, (const u32 *)deg, (u32)n, G->ptr.p);
    timer.launch(2);
    HIP_TRY(hipGetLastError());
    TRY(chip_read_back(ctx, G->ptr.p + n, sizeof(i64), &G->nedges));   // (the caller's host arrays are free again)
    TRY(G->idx.alloc((size_t)std::max<i64>(G->nedges, 1)));
    hipLaunchKernelGGL(rg_fill_kernel, dim3((unsigned)div_up(n, 4)), dim3(256), 0, s, bitmap, (u32)n, (u32)tiles,
                       (const i64 *)G->ptr.p, G->idx.p);
    timer.launch(1);
    timer.stop();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    timer.finish();
    return 0;
}

extern "C" int catchhip_redundancy_fetch(catchhip_ctx *ctx, const catchhip_redgraph *G, i64 *ptr, u32 *idx) {
    ARG_CHECK(ctx && G && ptr && G->ctx == ctx && (G->nedges == 0 || idx));
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(ptr, G->ptr.p, sizeof(i64) * ((size_t)G->n + 1), hipMemcpyDeviceToHost, ctx->stream));
    if (G->nedges)
        HIP_TRY(hipMemcpyAsync(idx, G->idx.p, sizeof(u32) * (size_t)G->nedges, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int catchhip_redundancy_destroy(catchhip_redgraph *G) {
    if (!G) return 0;
    PoolScope pool_scope(G->ctx);
    delete G;
    return 0;
}

extern "C" int catchhip_redundancy_naive(catchhip_ctx *ctx, const catchhip_redgraph *G, u8 *keep) {
    ARG_CHECK(ctx && G && G->ctx == ctx && (G->n == 0 || keep));
    if (G->n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope pool_scope(ctx);
    hipStream_t s = ctx->stream;
    const u32 n = (u32)G->n;
    DevBuf<u8> state, d_keep;
    DevBuf<u32> left;
    TRY(state.alloc(n));
    TRY(d_keep.alloc(n));
    TRY(left.alloc(RN_ROUNDS));
    TRY(chip_pinned_reserve(ctx, std::max<size_t>(n, sizeof(u32) * RN_ROUNDS)));
    HIP_TRY(hipMemsetAsync(state.p, 0, n, s));
    PhaseTimer timer(ctx, PHASE_NDF);
    const unsigned nb = (unsigned)div_up((i64)n, 256);
    u32 undecided = n;
    while (undecided) {
        HIP_TRY(hipMemsetAsync(left.p, 0, sizeof(u32) * RN_ROUNDS, s));
        for (int r = 0; r < RN_ROUNDS; ++r)
            hipLaunchKernelGGL(rn_round_kernel, dim3(nb), dim3(256), 0, s, (const i64 *)G->ptr.p, (const u32 *)G->idx.p, n,
                               state.p, left.p + r);
        timer.launch(RN_ROUNDS);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(ctx->h_big, left.p, sizeof(u32) * RN_ROUNDS, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const u32 *h_left = (const u32 *)ctx->h_big;
        const u32 before_last = h_left[RN_ROUNDS - 2];
        undecided = h_left[RN_ROUNDS - 1];
        if (undecided && before_last - undecided < RN_FEW) {
            // a long dependency chain (a path graph decides one or two vertices per round): walk it in order
            hipLaunchKernelGGL(rn_finish_kernel, dim3(1), dim3(RN_BLOCK), 0, s, (const i64 *)G->ptr.p,
                               (const u32 *)G->idx.p, n, state.p);
            timer.launch(1);
            undecided = 0;
        }
    }
    hipLaunchKernelGGL(rn_keep_kernel, dim3(nb), dim3(256), 0, s, (const u8 *)state.p, n, d_keep.p);
    timer.launch(1);
    timer.stop();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->h_big, d_keep.p, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    timer.finish();
    memcpy(keep, ctx->h_big, n);
    return 0;
}

extern "C" int catchhip_redundancy_rows(catchhip_ctx *ctx, const catchhip_redgraph *G, catchhip_rows **out, i64 *nrows) {
    ARG_CHECK(ctx && G && out && G->ctx == ctx);
    *out = nullptr;
    const i64 n = G->n, rows = G->nedges + n;
    if (rows >= ((i64)1 << 31)) {
        chip_set_error("redundancy_rows: %lld probes with %lld redundant pairs make %lld rows; the solver takes fewer "
                       "than 2^31", (long long)n, (long long)(G->nedges / 2), (long long)rows);
        return CATCHHIP_EINVAL;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope pool_scope(ctx);
    hipStream_t s = ctx->stream;
    std::unique_ptr<catchhip_rows> R(new catchhip_rows());
    R->ctx = ctx;
    R->n = rows;
    R->ngenomes = 1;
    R->total = 2 * n;
    R->lmax = rows ? 1 : 0;
    R->h_genome_off = {0, 2 * n};
    const u32 go[2] = {0u, (u32)(2 * n)};
    TRY(chip_rows_alloc_soa(R.get(), (size_t)rows));
    TRY(R->genome_off.alloc(2));
    HIP_TRY(hipMemcpyAsync(R->genome_off.p, go, sizeof(go), hipMemcpyHostToDevice, s));
    if (n)
        hipLaunchKernelGGL(rr_rows_kernel, dim3((unsigned)div_up(n, 4)), dim3(256), 0, s, (const i64 *)G->ptr.p,
                           (const u32 *)G->idx.p, (u32)n, R->set_id.p, R->univ.p, R->gs.p, R->ge.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    if (nrows) *nrows = rows;
    *out = R.release();
    return 0;
}
