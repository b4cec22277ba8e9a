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
#include "../../include/catchhip_cross.h"
#include "../../include/catchhip_redesign.h"
#include "cross_tile.h"

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

// the pair launch of either one-list entry
static void cd_pairs(hipStream_t s, const CdInput &in, bool graph, i64 n, i32 above, unsigned long long *best,
                     unsigned long long *bitmap) {
    const dim3 grid((unsigned)in.tiles, (unsigned)in.tiles);
    const u32 rowwords = (u32)in.tiles;
    if (in.W == 1) cd_launch_pairs<1>(s, grid, graph, in.fwd.p, in.rev.p, in.lens.p, (u32)n, (u32)in.npad, above, best, bitmap, rowwords);
    else if (in.W == 2) cd_launch_pairs<2>(s, grid, graph, in.fwd.p, in.rev.p, in.lens.p, (u32)n, (u32)in.npad, above, best, bitmap, rowwords);
    else cd_launch_pairs<4>(s, grid, graph, in.fwd.p, in.rev.p, in.lens.p, (u32)n, (u32)in.npad, above, best, bitmap, rowwords);
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

static void ca_against(hipStream_t s, dim3 grid, bool flags, const CdInput &A, u32 na, u32 per, const CdInput &B, u32 nb,
                       i32 above, unsigned long long *best, u8 *flag) {
    if (A.W == 1) ca_launch<1>(s, grid, flags, A, na, per, B, nb, above, best, flag);
    else if (A.W == 2) ca_launch<2>(s, grid, flags, A, na, per, B, nb, above, best, flag);
    else ca_launch<4>(s, grid, flags, A, na, per, B, nb, above, best, flag);
}

// the four entries: cross_tile.h's host side over this file's kernels
static const CdLaunch CD_LENGTH = {"cross_dimer", "cross_dimer_graph", "cross_against", "cross_against_flags", 1, cd_pairs,
                                   ca_against};

extern "C" int catchhip_cross_dimer(catchhip_ctx *ctx, const u8 *bytes, const i64 *off, i64 n, i32 *value, i32 *partner) {
    ARG_CHECK(ctx && off && n >= 0 && (n == 0 || (bytes && value && partner)));
    return cd_run_values(ctx, CD_LENGTH, bytes, off, n, value, partner);
}

extern "C" int catchhip_cross_dimer_graph(catchhip_ctx *ctx, const u8 *bytes, const i64 *off, i64 n, i32 above,
                                          catchhip_redgraph **out, i64 *nedges) {
    ARG_CHECK(ctx && out && off && n >= 0 && (n == 0 || bytes));
    return cd_run_graph(ctx, CD_LENGTH, bytes, off, n, above, out, nedges);
}

extern "C" int catchhip_cross_against(catchhip_ctx *ctx, const u8 *b_bytes, const i64 *b_off, i64 nb, const u8 *a_bytes,
                                      const i64 *a_off, i64 na, i32 *value, i32 *partner) {
    ARG_CHECK(ctx && na >= 0 && nb >= 0 && (nb == 0 || (b_bytes && b_off && value && partner)) &&
              (na == 0 || (a_bytes && a_off)));
    return ca_run(ctx, CD_LENGTH, b_bytes, b_off, nb, a_bytes, a_off, na, false, 0, value, partner, nullptr);
}

extern "C" int catchhip_cross_against_flags(catchhip_ctx *ctx, const u8 *b_bytes, const i64 *b_off, i64 nb, const u8 *a_bytes,
                                            const i64 *a_off, i64 na, i32 above, u8 *flag) {
    ARG_CHECK(ctx && na >= 0 && nb >= 0 && (nb == 0 || (b_bytes && b_off && flag)) && (na == 0 || (a_bytes && a_off)));
    return ca_run(ctx, CD_LENGTH, b_bytes, b_off, nb, a_bytes, a_off, na, true, above, nullptr, nullptr, flag);
}
