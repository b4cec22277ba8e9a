// Cross-dimers: how far two DIFFERENT records of a list pair with each other, antiparallel
// (catchhip_cross_dimer / catchhip_cross_dimer_graph; catch_amd/filter/cross_dimer.py has the definition).
//
// run(s, t) is the longest run of cells pairs(x, y) = "s[x] and t[y] are bases and complementary" along an
// antidiagonal x + y = c of the Ls x Lt table -- measure.hip's dimer with the two copies of one candidate replaced by
// two records.  All n (n - 1) / 2 pairs are evaluated, in redundant.hip's organisation: a block owns a 64 x 64 tile of
// the upper triangle of the pair matrix, diagonal tiles included, and stages both sides' bit planes in LDS.
//
// Planes.  A record becomes three planes V / B0 / B1 in planes.h's coding (a base; bits 1 and 2 of the byte, so that a
// base and its complement agree in B0 and differ in B1) of W 64-bit words, W in {1, 2, 4} by the longest record, and a
// second time bit-reversed over the 64 W bits.  The row side of a tile stages the plain planes, the column side the
// reversed ones: cell (x, c - x) reads bit c - x of the column record, which is bit x + d of its reversed planes,
// d = 64 W - 1 - c -- ONE shift for the whole antidiagonal.  For d >= 0 the reversed planes move down by d, for d < 0
// the row's planes move down by -d (the cells then sit at bit x + d); either way a funnel shift of two LDS words per
// plane, the upper W words of a staged plane being zero, and
//     m = (B1 ^ rB1) & ~(B0 ^ rB0) & V & rV
// has a 1 exactly at the cells of the antidiagonal: whatever is no base, or lies outside a record, has V = 0.
//
// Run search.  run = the longest run of 1-bits in the 64 W bits of m, over all antidiagonals.  With a best t in hand,
// "is there a run longer than t" is six AND-shifts over the words (the run in hand grows 1 -> min(t + 1, 64); the bits
// that fall off a word come in from the next one), and only an antidiagonal that passes is measured exactly, by single
// steps from there.  An antidiagonal of at most t cells is never looked at: c runs from t to la + lb - 2 - t.
//
// Order and bests.  Step k of a tile pairs column `lane` with row (lane + k) mod 64, a wave taking 16 steps: every row
// and every column meets one partner per step, so the bests of BOTH sides, kept as keys in LDS, rise as the tile goes
// on, and a pair is searched only above what would still change either side.  A key is
//     (value << 32) | (0xFFFFFFFF - partner),
// so that the larger key is the larger value and, of equal values, the smaller partner; a tile starts from the keys
// the tiles before it left in global memory and merges its own with one atomic maximum per record.  A threshold read
// too early is only lower than it could be: what is searched varies from run to run, the maximum does not.
// Each unordered pair is evaluated once (i < j) and its value offered to both records.
//
// The graph entry is the same kernel with the threshold fixed at `above` and an exit at the first run beyond it; its
// hits are bits of the adjacency bitmap, collected per tile in LDS, and the graph is redundant.hip's from there.
//
// One list against another (catchhip_cross_against / _flags) is at the end of the file: the same planes and the same
// cd_pair, a tile of B held against the stream of A's tiles.
#include <algorithm>

#include "../../include/catchhip_cross.h"
#include "../../include/catchhip_redesign.h"
#include "redgraph.h"

#define CD_MAXN (RG_TILE * 16384)      // records of one catchhip_cross_dimer call: 16,384 tiles a side

// one 64-character word of a record's three planes
__host__ __device__ static inline void cd_pack_word(const u8 *chars, u32 len, int w, u64 *v, u64 *b0, u64 *b1) {
    u64 xv = 0, x0 = 0, x1 = 0;
    const u32 lo = (u32)w * 64, hi = len < lo + 64 ? len : lo + 64;
    for (u32 i = lo; i < hi; ++i) {
        const u32 c = chars[i];
        xv |= (u64)(c == 'A' || c == 'C' || c == 'G' || c == 'T') << (i - lo);
        x0 |= (u64)((c >> 1) & 1u) << (i - lo);
        x1 |= (u64)((c >> 2) & 1u) << (i - lo);
    }
    *v = xv; *b0 = x0; *b1 = x1;
}

// fwd / rev[(plane * W + w) * npad + record]; word w of a reversed plane is word W - 1 - w of the plain one with its
// bits reversed.  Records beyond n stay zero.
__global__ void cd_pack_kernel(const u8 *__restrict__ bytes, const i64 *__restrict__ off, u32 n, u32 npad, int W,
                               u64 *__restrict__ fwd, u64 *__restrict__ rev, u32 *__restrict__ lens) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const i64 a = off[p];
    const u32 len = (u32)(off[p + 1] - a);
    lens[p] = len;
    for (int w = 0; w < W; ++w) {
        u64 v, b0, b1;
        cd_pack_word(bytes + a, len, w, &v, &b0, &b1);
        fwd[((size_t)(0 * W + w)) * npad + p] = v;
        fwd[((size_t)(1 * W + w)) * npad + p] = b0;
        fwd[((size_t)(2 * W + w)) * npad + p] = b1;
        rev[((size_t)(0 * W + (W - 1 - w))) * npad + p] = __brevll(v);
        rev[((size_t)(1 * W + (W - 1 - w))) * npad + p] = __brevll(b0);
        rev[((size_t)(2 * W + (W - 1 - w))) * npad + p] = __brevll(b1);
    }
}

// x &= x >> s over the 64 W bits (0 <= s <= 63; s = 0 leaves x as it is)
template <int W> __host__ __device__ __forceinline__ void cd_and_shift(u64 (&x)[W], u32 s) {
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const u64 hi = w + 1 < W ? x[w + 1] : 0ull;      // (not yet changed: w ascends)
        x[w] &= (x[w] >> s) | ((hi << 1) << (63u - s));
    }
}

// planes.h's RunShifts over 64 W bits: six steps that grow the run in hand 1 -> want <= 64
struct CdSteps {
    u32 want, s0, s1, s2, s3, s4, s5;
    __host__ __device__ __forceinline__ void aim(u32 w) {
        want = w;
        u32 have = 1, s[6];
        for (int k = 0; k < 6; ++k) {                       // (unrolled: s[] stays in registers)
            s[k] = have >= want ? 0u : (have < want - have ? have : want - have);
            have += s[k];
        }
        s0 = s[0]; s1 = s[1]; s2 = s[2]; s3 = s[3]; s4 = s[4]; s5 = s[5];
    }
    // afterwards bit b of x <=> bits b .. b + want - 1 of what x was
    template <int W> __host__ __device__ __forceinline__ void inside(u64 (&x)[W]) const {
        cd_and_shift<W>(x, s0);
        cd_and_shift<W>(x, s1);
        cd_and_shift<W>(x, s2);
        cd_and_shift<W>(x, s3);
        cd_and_shift<W>(x, s4);
        cd_and_shift<W>(x, s5);
    }
};

template <int W> __host__ __device__ __forceinline__ bool cd_any(const u64 (&x)[W]) {
    u64 o = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) o |= x[w];
    return o != 0;
}

// run(a, b) where it exceeds t, else some value <= t.  a points at word 0 of plane V of the row record's plain
// planes, rb at the same of the column record's reversed planes, both in a tile's layout [plane][2 W words][RG_TILE]
// with words W .. 2 W - 1 zero (a shifted read never leaves the array); la / lb are the lengths.  GRAPH: t + 1 at the
// first run longer than t.
template <int W, bool GRAPH>
__host__ __device__ static inline int cd_pair(const u64 *a, const u64 *rb, int la, int lb, int t) {
    int best = 0;
    if ((la < lb ? la : lb) <= t) return 0;
    CdSteps steps;
    steps.aim((u32)(t < 63 ? t + 1 : 64));
    for (int c = t; c <= la + lb - 2 - t; ++c) {
        const int d = 64 * W - 1 - c;                        // |d| <= 64 W - 1: la + lb - 2 <= 128 W - 2
        const int s = d >= 0 ? d : -d;
        const int ws = s >> 6;
        const u32 bs = (u32)s & 63u;
        const u64 *sh = d >= 0 ? rb : a, *un = d >= 0 ? a : rb;
        u64 m[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            u64 p[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                const u64 lo = sh[(size_t)(pl * 2 * W + w + ws) * RG_TILE], hi = sh[(size_t)(pl * 2 * W + w + ws + 1) * RG_TILE];
                p[pl] = (lo >> bs) | ((hi << 1) << (63u - bs));
            }
            m[w] = (p[2] ^ un[(size_t)(2 * 2 * W + w) * RG_TILE]) & ~(p[1] ^ un[(size_t)(1 * 2 * W + w) * RG_TILE]) & p[0] &
                   un[(size_t)w * RG_TILE];
        }
        steps.inside<W>(m);
        if (!cd_any<W>(m)) continue;
        if (GRAPH && t < 64) return t + 1;
        // a run of steps.want or more: every further single step is one more
        int len = (int)steps.want - 1;
        do {
            ++len;
            cd_and_shift<W>(m, 1u);
        } while (cd_any<W>(m));
        if (len > t) {                                       // (want stops at 64: a run of 64 .. t changes nothing)
            if (GRAPH) return t + 1;
            best = t = len;
            steps.aim((u32)(t < 63 ? t + 1 : 64));
        }
    }
    return best;
}

// what a pair with `other` as the partner must exceed to change the record that holds `key`
__device__ __forceinline__ int cd_threshold(unsigned long long key, u32 other) {
    const int v = (int)(key >> 32);
    const u32 partner = 0xFFFFFFFFu - (u32)key;
    return v == 0 ? 0 : (other < partner ? v - 1 : v);
}

// One 64 x 64 tile of pairs (rows ti * 64 .., columns tj * 64 .., ti <= tj); pair (gi, gj) counts when gi < gj < n:
// a diagonal tile leaves out a record's own pairing and keeps equal records at different indices.
// s_acc: a side's keys (values) or adjacency bits (GRAPH), row side 0, column side 1.
template <int W, bool GRAPH>
__global__ void __launch_bounds__(RG_BLOCK)
cd_pairs_kernel(const u64 *__restrict__ fwd, const u64 *__restrict__ rev, const u32 *__restrict__ lens, u32 n, u32 npad,
                i32 above, unsigned long long *best, unsigned long long *bitmap, u32 rowwords) {
    const u32 ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    __shared__ u64 s_pl[2][3][2 * W][RG_TILE];
    __shared__ u32 s_len[2][RG_TILE];
    __shared__ unsigned long long s_acc[2][RG_TILE];
    for (u32 t = threadIdx.x; t < 2 * 3 * 2 * W * RG_TILE; t += RG_BLOCK) {
        const u32 pr = t % RG_TILE, w = (t / RG_TILE) % (2 * W), pl = (t / (RG_TILE * 2 * W)) % 3, side = t / (RG_TILE * 2 * W * 3);
        const u32 g = (side ? tj : ti) * RG_TILE + pr;      // < npad
        s_pl[side][pl][w][pr] = w < (u32)W ? (side ? rev : fwd)[((size_t)(pl * W + w)) * npad + g] : 0ull;
    }
    if (threadIdx.x < 2 * RG_TILE) {
        const u32 side = threadIdx.x / RG_TILE, pr = threadIdx.x % RG_TILE;
        const u32 g = (side ? tj : ti) * RG_TILE + pr;
        s_len[side][pr] = lens[g];
        s_acc[side][pr] = GRAPH ? 0ull : __hip_atomic_load(best + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 gj = tj * RG_TILE + lane;
    const int lb = (int)s_len[1][lane];
    for (u32 k = wave * (RG_TILE * 64 / RG_BLOCK); k < (wave + 1) * (RG_TILE * 64 / RG_BLOCK); ++k) {
        const u32 r = (lane + k) & (RG_TILE - 1);
        const u32 gi = ti * RG_TILE + r;
        if (!(gi < gj && gj < n)) continue;
        int t = above;
        if (!GRAPH) {
            const int tr = cd_threshold(__hip_atomic_load(&s_acc[0][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), gj);
            const int tc = cd_threshold(__hip_atomic_load(&s_acc[1][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), gi);
            t = tr < tc ? tr : tc;
        }
        const int v = cd_pair<W, GRAPH>(&s_pl[0][0][0][r], &s_pl[1][0][0][lane], (int)s_len[0][r], lb, t);
        if (v <= t) continue;
        if (GRAPH) {
            atomicOr(&s_acc[0][r], 1ull << lane);
            atomicOr(&s_acc[1][lane], 1ull << r);
        } else {
            atomicMax(&s_acc[0][r], ((unsigned long long)(u32)v << 32) | (unsigned long long)(0xFFFFFFFFu - gj));
            atomicMax(&s_acc[1][lane], ((unsigned long long)(u32)v << 32) | (unsigned long long)(0xFFFFFFFFu - gi));
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * RG_TILE) {
        const u32 side = threadIdx.x / RG_TILE, pr = threadIdx.x % RG_TILE;
        const u32 g = (side ? tj : ti) * RG_TILE + pr;
        const unsigned long long acc = s_acc[side][pr];
        if (g < n && acc) {
            if (GRAPH) atomicOr(&bitmap[(size_t)g * rowwords + (side ? ti : tj)], acc);
            else atomicMax(&best[g], acc);
        }
    }
}

__global__ void cd_result_kernel(const unsigned long long *__restrict__ best, u32 n, i32 *__restrict__ value,
                                 i32 *__restrict__ partner) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = best[i];
    const i32 v = (i32)(key >> 32);
    value[i] = v;
    partner[i] = v ? (i32)(0xFFFFFFFFu - (u32)key) : -1;
}

template <int W>
static void cd_launch_pairs(hipStream_t s, dim3 grid, bool graph, const u64 *fwd, const u64 *rev, const u32 *lens, u32 n,
                            u32 npad, i32 above, unsigned long long *best, unsigned long long *bitmap, u32 rowwords) {
    if (graph)
        hipLaunchKernelGGL((cd_pairs_kernel<W, true>), grid, dim3(RG_BLOCK), 0, s, fwd, rev, lens, n, npad, above, best, bitmap,
                           rowwords);
    else
        hipLaunchKernelGGL((cd_pairs_kernel<W, false>), grid, dim3(RG_BLOCK), 0, s, fwd, rev, lens, n, npad, above, best, bitmap,
                           rowwords);
}

// the records of a call on the device, packed: any bytes, 0 .. RG_MAXLEN characters each
struct CdInput {
    i64 tiles = 0, npad = 0;
    int W = 1;
    DevBuf<u8> d_bytes;
    DevBuf<i64> d_off;
    DevBuf<u64> fwd, rev;
    DevBuf<u32> lens;
};

static int cd_check(const char *who, const i64 *off, i64 n, int *W) {
    i64 maxlen = 0;
    for (i64 i = 0; i < n; ++i) {
        const i64 len = off[i + 1] - off[i];
        if (len < 0) { chip_set_error("%s: offsets of record %lld decrease", who, (long long)i); return CATCHHIP_EINVAL; }
        if (len > RG_MAXLEN) {
            chip_set_error("%s: record %lld has %lld characters; the kernel pairs at most %d", who, (long long)i,
                           (long long)len, RG_MAXLEN);
            return CATCHHIP_EINVAL;
        }
        maxlen = std::max(maxlen, len);
    }
    *W = maxlen <= 64 ? 1 : maxlen <= 128 ? 2 : 4;
    return 0;
}

// uploads n >= 1 records on ctx->stream and clears what cd_pack fills; in->W is set
static int cd_stage(catchhip_ctx *ctx, const u8 *bytes, const i64 *off, i64 n, CdInput *in) {
    hipStream_t s = ctx->stream;
    const int W = in->W;
    in->tiles = div_up(n, RG_TILE);
    in->npad = in->tiles * RG_TILE;
    const i64 npad = in->npad, total = off[n] - off[0];
    TRY(in->d_bytes.alloc((size_t)total + 1));
    TRY(in->d_off.alloc((size_t)n + 1));
    TRY(in->fwd.alloc((size_t)3 * W * npad));
    TRY(in->rev.alloc((size_t)3 * W * npad));
    TRY(in->lens.alloc((size_t)npad));
    // (offsets relative to the first byte handed over)
    std::vector<i64> rel((size_t)n + 1);
    for (i64 i = 0; i <= n; ++i) rel[i] = off[i] - off[0];
    if (total) HIP_TRY(hipMemcpyAsync(in->d_bytes.p, bytes + off[0], (size_t)total, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(in->d_off.p, rel.data(), sizeof(i64) * ((size_t)n + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(in->fwd.p, 0, sizeof(u64) * (size_t)3 * W * npad, s));
    HIP_TRY(hipMemsetAsync(in->rev.p, 0, sizeof(u64) * (size_t)3 * W * npad, s));
    HIP_TRY(hipMemsetAsync(in->lens.p, 0, sizeof(u32) * (size_t)npad, s));
    HIP_TRY(hipStreamSynchronize(s));       // (rel[] goes out of scope)
    return 0;
}

// the two launches of either entry: pack, pairs
static void cd_pairs(hipStream_t s, const CdInput &in, bool graph, i64 n, i32 above, unsigned long long *best,
                     unsigned long long *bitmap) {
    hipLaunchKernelGGL(cd_pack_kernel, dim3((unsigned)div_up(n, 256)), dim3(256), 0, s, (const u8 *)in.d_bytes.p,
                       (const i64 *)in.d_off.p, (u32)n, (u32)in.npad, in.W, in.fwd.p, in.rev.p, in.lens.p);
    const dim3 grid((unsigned)in.tiles, (unsigned)in.tiles);
    const u32 rowwords = (u32)in.tiles;
    if (in.W == 1) cd_launch_pairs<1>(s, grid, graph, in.fwd.p, in.rev.p, in.lens.p, (u32)n, (u32)in.npad, above, best, bitmap, rowwords);
    else if (in.W == 2) cd_launch_pairs<2>(s, grid, graph, in.fwd.p, in.rev.p, in.lens.p, (u32)n, (u32)in.npad, above, best, bitmap, rowwords);
    else cd_launch_pairs<4>(s, grid, graph, in.fwd.p, in.rev.p, in.lens.p, (u32)n, (u32)in.npad, above, best, bitmap, rowwords);
}

extern "C" int catchhip_cross_dimer(catchhip_ctx *ctx, const u8 *bytes, const i64 *off, i64 n, i32 *value, i32 *partner) {
    ARG_CHECK(ctx && off && n >= 0 && (n == 0 || (bytes && value && partner)));
    if (n > CD_MAXN) {
        chip_set_error("cross_dimer: %lld records; one call pairs at most %d (%d tiles a side)", (long long)n, CD_MAXN,
                       CD_MAXN / RG_TILE);
        return CATCHHIP_EINVAL;
    }
    CdInput in;
    TRY(cd_check("cross_dimer", off, n, &in.W));
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope pool_scope(ctx);
    hipStream_t s = ctx->stream;
    DevBuf<unsigned long long> best;
    DevBuf<i32> d_out;
    TRY(best.alloc((size_t)div_up(n, RG_TILE) * RG_TILE));
    TRY(d_out.alloc((size_t)2 * n));
    HIP_TRY(hipMemsetAsync(best.p, 0, sizeof(unsigned long long) * (size_t)div_up(n, RG_TILE) * RG_TILE, s));
    TRY(cd_stage(ctx, bytes, off, n, &in));
    PhaseTimer timer(ctx, PHASE_NDF);
    cd_pairs(s, in, false, n, 0, best.p, nullptr);
    hipLaunchKernelGGL(cd_result_kernel, dim3((unsigned)div_up(n, 256)), dim3(256), 0, s, (const unsigned long long *)best.p,
                       (u32)n, d_out.p, d_out.p + n);
    timer.launch(3);
    timer.stop();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(value, d_out.p, sizeof(i32) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(partner, d_out.p + n, sizeof(i32) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    timer.finish();
    return 0;
}

extern "C" int catchhip_cross_dimer_graph(catchhip_ctx *ctx, const u8 *bytes, const i64 *off, i64 n, i32 above,
                                          catchhip_redgraph **out, i64 *nedges) {
    ARG_CHECK(ctx && out && off && n >= 0 && (n == 0 || bytes));
    *out = nullptr;
    if (above < 1) {
        chip_set_error("cross_dimer_graph: the threshold must be at least 1 (%d)", above);
        return CATCHHIP_EINVAL;
    }
    CdInput in;
    TRY(cd_check("cross_dimer_graph", off, n, &in.W));
    HIP_TRY(hipSetDevice(ctx->device));
    const i64 tiles = div_up(std::max<i64>(n, 1), RG_TILE);
    const double bitmap_bytes = (double)n * (double)tiles * 8.0;
    if (tiles > 65535 || bitmap_bytes > 0.5 * (double)chip_pool_soft_limit()) {
        chip_set_error("cross_dimer_graph: %lld records: the adjacency bitmap (%.1f GB) is larger than half of what the "
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
    DevBuf<u32> deg;
    DevBuf<unsigned long long> bitmap;
    TRY(deg.alloc((size_t)n));
    TRY(bitmap.alloc((size_t)n * tiles));
    HIP_TRY(hipMemsetAsync(bitmap.p, 0, sizeof(unsigned long long) * (size_t)n * tiles, s));
    TRY(cd_stage(ctx, bytes, off, n, &in));
    PhaseTimer timer(ctx, PHASE_NDF);
    cd_pairs(s, in, true, n, above, nullptr, bitmap.p);
    timer.launch(2);
    TRY(chip_redgraph_from_bitmap(ctx, timer, bitmap.p, tiles, deg.p, G.get()));
    if (nedges) *nedges = G->nedges;
    *out = G.release();
    return 0;
}

// ---- one list against another (catchhip_cross_against / _flags; include/catchhip_redesign.h) --------------------------
// cross_against(b, A) = max over a in A of run(b, a), nothing exempted.  A block owns one tile of 64 records of B,
// staged once on the reversed (column) side, and streams a range of A's tiles through the plain (row) side with the
// one-list kernel's skewed order: step k pairs column `lane` with row (lane + k) mod 64, a wave taking 16 steps of
// every tile.  A column's best (a key as above, the partner an index into A) or flag lives in LDS for the whole
// stream and goes out once at the end: by atomic maximum, since gridDim.y blocks share a B tile when B alone would not
// fill the device (block y takes A's tiles y * per .. ), or as a byte that is only ever written as 1.  What a block
// searches depends on the keys it read; the maximum, and the smallest partner of equal values, do not.
// FLAGS: the threshold is `above` throughout, a pair ends at its first run beyond it, a flagged column is skipped and
// a tile whose columns are all flagged leaves the stream.
template <int W, bool FLAGS>
__global__ void __launch_bounds__(RG_BLOCK)
cd_against_kernel(const u64 *__restrict__ a_fwd, const u32 *__restrict__ a_lens, u32 na, u32 a_npad, u32 a_tiles, u32 per,
                  const u64 *__restrict__ b_rev, const u32 *__restrict__ b_lens, u32 nb, u32 b_npad, i32 above,
                  unsigned long long *best, u8 *flag) {
    const u32 tb = blockIdx.x;
    const u32 t_lo = blockIdx.y * per, t_hi = t_lo + per < a_tiles ? t_lo + per : a_tiles;
    if (t_lo >= t_hi) return;
    __shared__ u64 s_pl[2][3][2 * W][RG_TILE];
    __shared__ u32 s_len[2][RG_TILE];
    __shared__ unsigned long long s_acc[RG_TILE];
    for (u32 t = threadIdx.x; t < 3 * 2 * W * RG_TILE; t += RG_BLOCK) {
        const u32 pr = t % RG_TILE, w = (t / RG_TILE) % (2 * W), pl = t / (RG_TILE * 2 * W);
        s_pl[1][pl][w][pr] = w < (u32)W ? b_rev[((size_t)(pl * W + w)) * b_npad + tb * RG_TILE + pr] : 0ull;   // < b_npad
    }
    if (threadIdx.x < RG_TILE) {
        const u32 g = tb * RG_TILE + threadIdx.x;
        s_len[1][threadIdx.x] = b_lens[g];
        s_acc[threadIdx.x] = FLAGS ? 0ull : __hip_atomic_load(best + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 gb = tb * RG_TILE + lane;
    for (u32 ta = t_lo; ta < t_hi; ++ta) {
        for (u32 t = threadIdx.x; t < 3 * 2 * W * RG_TILE; t += RG_BLOCK) {
            const u32 pr = t % RG_TILE, w = (t / RG_TILE) % (2 * W), pl = t / (RG_TILE * 2 * W);
            s_pl[0][pl][w][pr] = w < (u32)W ? a_fwd[((size_t)(pl * W + w)) * a_npad + ta * RG_TILE + pr] : 0ull;   // < a_npad
        }
        if (threadIdx.x < RG_TILE) s_len[0][threadIdx.x] = a_lens[ta * RG_TILE + threadIdx.x];
        __syncthreads();
        const int lb = (int)s_len[1][lane];
        for (u32 k = wave * (RG_TILE * 64 / RG_BLOCK); k < (wave + 1) * (RG_TILE * 64 / RG_BLOCK); ++k) {
            const u32 r = (lane + k) & (RG_TILE - 1);
            const u32 ga = ta * RG_TILE + r;
            if (!(ga < na && gb < nb)) continue;
            const unsigned long long mine = __hip_atomic_load(&s_acc[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (FLAGS && mine) continue;
            const int t = FLAGS ? above : cd_threshold(mine, ga);
            const int v = cd_pair<W, FLAGS>(&s_pl[0][0][0][r], &s_pl[1][0][0][lane], (int)s_len[0][r], lb, t);
            if (v <= t) continue;
            if (FLAGS) __hip_atomic_store(&s_acc[lane], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else atomicMax(&s_acc[lane], ((unsigned long long)(u32)v << 32) | (unsigned long long)(0xFFFFFFFFu - ga));
        }
        // (the barrier in front of the next tile's staging; a flag set behind this read costs one more tile, no more)
        const int done = FLAGS && (gb >= nb || __hip_atomic_load(&s_acc[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        if (__syncthreads_and(done)) break;
    }
    __syncthreads();
    if (threadIdx.x < RG_TILE) {
        const u32 g = tb * RG_TILE + threadIdx.x;
        const unsigned long long acc = s_acc[threadIdx.x];
        if (g < nb && acc) {
            if (FLAGS) flag[g] = 1;
            else atomicMax(&best[g], acc);
        }
    }
}

#define CA_MAXN ((i64)1 << 30)         // records of either list: the padded count and the tiles stay 32-bit
// Blocks wanted before A's range is split no further: 256 CUs hold 8 blocks of 256 threads each, and blocks end at
// uneven times (the early exits), so the device is level only with several rounds of them -- at 1,563 B tiles and one
// range a CU got 6 or 7 blocks, each as long as the whole stream of A: 1.63 x 10^9 pairs/s for the flags of 100,000
// random 100-mers against 1,000, 2.07 x 10^9 at the 6 ranges this asks for (tools/cross_against_profile.py).
#define CA_FILL 8192

template <int W>
static void ca_launch(hipStream_t s, dim3 grid, bool flags, const CdInput &A, u32 na, u32 per, const CdInput &B, u32 nb,
                      i32 above, unsigned long long *best, u8 *flag) {
    if (flags)
        hipLaunchKernelGGL((cd_against_kernel<W, true>), grid, dim3(RG_BLOCK), 0, s, (const u64 *)A.fwd.p, (const u32 *)A.lens.p,
                           na, (u32)A.npad, (u32)A.tiles, per, (const u64 *)B.rev.p, (const u32 *)B.lens.p, nb, (u32)B.npad,
                           above, best, flag);
    else
        hipLaunchKernelGGL((cd_against_kernel<W, false>), grid, dim3(RG_BLOCK), 0, s, (const u64 *)A.fwd.p, (const u32 *)A.lens.p,
                           na, (u32)A.npad, (u32)A.tiles, per, (const u64 *)B.rev.p, (const u32 *)B.lens.p, nb, (u32)B.npad,
                           above, best, flag);
}

// both entries: checks, both lists packed with one W, the stream of A's tiles; value / partner or flag on the host
static int ca_run(catchhip_ctx *ctx, const char *who, const u8 *b_bytes, const i64 *b_off, i64 nb, const u8 *a_bytes,
                  const i64 *a_off, i64 na, bool flags, i32 above, i32 *value, i32 *partner, u8 *flag) {
    if (flags && above < 1) {
        chip_set_error("%s: the threshold must be at least 1 (%d)", who, above);
        return CATCHHIP_EINVAL;
    }
    if (na > CA_MAXN || nb > CA_MAXN) {
        chip_set_error("%s: %lld records against %lld; one call takes at most %lld in a list", who, (long long)nb,
                       (long long)na, (long long)CA_MAXN);
        return CATCHHIP_EINVAL;
    }
    CdInput A, B;
    TRY(cd_check(who, b_off, nb, &B.W));
    TRY(cd_check(who, a_off, na, &A.W));
    for (i64 i = 0; i < nb; ++i) {                           // an empty A, or nothing to ask
        if (flags) flag[i] = 0;
        else { value[i] = 0; partner[i] = -1; }
    }
    if (na == 0 || nb == 0) return 0;
    A.W = B.W = std::max(A.W, B.W);
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope pool_scope(ctx);
    hipStream_t s = ctx->stream;
    const i64 b_npad = div_up(nb, RG_TILE) * RG_TILE;
    DevBuf<unsigned long long> best;
    DevBuf<i32> d_out;
    DevBuf<u8> d_flag;
    if (flags) {
        TRY(d_flag.alloc((size_t)b_npad));
        HIP_TRY(hipMemsetAsync(d_flag.p, 0, (size_t)b_npad, s));
    } else {
        TRY(best.alloc((size_t)b_npad));
        TRY(d_out.alloc((size_t)2 * nb));
        HIP_TRY(hipMemsetAsync(best.p, 0, sizeof(unsigned long long) * (size_t)b_npad, s));
    }
    TRY(cd_stage(ctx, a_bytes, a_off, na, &A));
    TRY(cd_stage(ctx, b_bytes, b_off, nb, &B));
    // A's tiles in gridDim.y ranges of `per`: one range while B's tiles fill the device by themselves
    const i64 want = std::min<i64>(std::min<i64>(A.tiles, 65535), std::max<i64>(1, div_up((i64)CA_FILL, B.tiles)));
    const u32 per = (u32)div_up(A.tiles, want);
    const dim3 grid((unsigned)B.tiles, (unsigned)div_up(A.tiles, (i64)per));
    PhaseTimer timer(ctx, PHASE_NDF);
    hipLaunchKernelGGL(cd_pack_kernel, dim3((unsigned)div_up(na, 256)), dim3(256), 0, s, (const u8 *)A.d_bytes.p,
                       (const i64 *)A.d_off.p, (u32)na, (u32)A.npad, A.W, A.fwd.p, A.rev.p, A.lens.p);
    hipLaunchKernelGGL(cd_pack_kernel, dim3((unsigned)div_up(nb, 256)), dim3(256), 0, s, (const u8 *)B.d_bytes.p,
                       (const i64 *)B.d_off.p, (u32)nb, (u32)B.npad, B.W, B.fwd.p, B.rev.p, B.lens.p);
    if (A.W == 1) ca_launch<1>(s, grid, flags, A, (u32)na, per, B, (u32)nb, above, best.p, d_flag.p);
    else if (A.W == 2) ca_launch<2>(s, grid, flags, A, (u32)na, per, B, (u32)nb, above, best.p, d_flag.p);
    else ca_launch<4>(s, grid, flags, A, (u32)na, per, B, (u32)nb, above, best.p, d_flag.p);
    if (!flags)
        hipLaunchKernelGGL(cd_result_kernel, dim3((unsigned)div_up(nb, 256)), dim3(256), 0, s,
                           (const unsigned long long *)best.p, (u32)nb, d_out.p, d_out.p + nb);
    timer.launch(flags ? 3 : 4);
    timer.stop();
    HIP_TRY(hipGetLastError());
    if (flags) {
        HIP_TRY(hipMemcpyAsync(flag, d_flag.p, (size_t)nb, hipMemcpyDeviceToHost, s));
    } else {
        HIP_TRY(hipMemcpyAsync(value, d_out.p, sizeof(i32) * (size_t)nb, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(partner, d_out.p + nb, sizeof(i32) * (size_t)nb, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    timer.finish();
    return 0;
}

extern "C" int catchhip_cross_against(catchhip_ctx *ctx, const u8 *b_bytes, const i64 *b_off, i64 nb, const u8 *a_bytes,
                                      const i64 *a_off, i64 na, i32 *value, i32 *partner) {
    ARG_CHECK(ctx && na >= 0 && nb >= 0 && (nb == 0 || (b_bytes && b_off && value && partner)) &&
              (na == 0 || (a_bytes && a_off)));
    return ca_run(ctx, "cross_against", b_bytes, b_off, nb, a_bytes, a_off, na, false, 0, value, partner, nullptr);
}

extern "C" int catchhip_cross_against_flags(catchhip_ctx *ctx, const u8 *b_bytes, const i64 *b_off, i64 nb, const u8 *a_bytes,
                                            const i64 *a_off, i64 na, i32 above, u8 *flag) {
    ARG_CHECK(ctx && na >= 0 && nb >= 0 && (nb == 0 || (b_bytes && b_off && flag)) && (na == 0 || (a_bytes && a_off)));
    return ca_run(ctx, "cross_against_flags", b_bytes, b_off, nb, a_bytes, a_off, na, true, above, nullptr, nullptr, flag);
}
