// Everything of cross.hip's organisation but the pair function (cross.hip: the length of a pairing; duplex.hip: its
// nearest-neighbour stability): the packing of records into bit planes, an antidiagonal's match word, the AND-shift
// run search, the keys, the two tile kernels with their launchers, the staging of a call's records and the host side
// of the four entries.  A file brings a pair RULE, which says three things:
//   PREFIX, prefix<W>(a, q)             whether a block stages u16 s_q[64 W][RG_TILE] beside a row tile's planes, and
//                                       what fills one record's column of it (asked for only where PREFIX)
//   pair<W, FIRST>(a, rb, q, la, lb, t) the pair's value where it exceeds t, else anything <= t; FIRST: any value
//                                       beyond t, at the first run that has one
//   MIN_ABOVE, VALUES / GRAPH / AGAINST / FLAGS   the smallest `above` of its graph and flags entries, their names
// cross.hip's header comment has the organisation.
#pragma once
#include <algorithm>
#include <memory>
#include <vector>

#include "redgraph.h"

#define CD_MAXN (RG_TILE * 16384)      // records of one one-list values call: 16,384 tiles a side

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
static __global__ void cd_pack_kernel(const u8 *__restrict__ bytes, const i64 *__restrict__ off, u32 n, u32 npad, int W,
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

// The match word of antidiagonal c, d = 64 W - 1 - c.  a points at word 0 of plane V of the row record's plain planes,
// rb at the same of the column record's reversed planes, both in a tile's layout [plane][2 W words][RG_TILE] with
// words W .. 2 W - 1 zero (a shifted read never leaves the array).  For d >= 0 bit x of m is cell (x, c - x), for
// d < 0 bit x is cell (x - d, c - x + d): the row's planes are then the shifted ones.  (It takes c, not d: compiled
// on its own in front of a pair function, it then yields the code that the same lines give inside cd_pair's loop.)
template <int W>
__host__ __device__ __forceinline__ void cd_match(const u64 *a, const u64 *rb, int c, u64 (&m)[W]) {
    const int d = 64 * W - 1 - c;                            // |d| <= 64 W - 1: la + lb - 2 <= 128 W - 2
    const int s = d >= 0 ? d : -d;
    const int ws = s >> 6;
    const u32 bs = (u32)s & 63u;
    const u64 *sh = d >= 0 ? rb : a, *un = d >= 0 ? a : rb;
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
}

// what a pair with `other` as the partner must exceed to change the record that holds `key`
__device__ __forceinline__ int cd_threshold(unsigned long long key, u32 other) {
    const int v = (int)(key >> 32);
    const u32 partner = 0xFFFFFFFFu - (u32)key;
    return v == 0 ? 0 : (other < partner ? v - 1 : v);
}

static __global__ void cd_result_kernel(const unsigned long long *__restrict__ best, u32 n, i32 *__restrict__ value,
                                        i32 *__restrict__ partner) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = best[i];
    const i32 v = (i32)(key >> 32);
    value[i] = v;
    partner[i] = v ? (i32)(0xFFFFFFFFu - (u32)key) : -1;
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

// One 64 x 64 tile of pairs (rows ti * 64 .., columns tj * 64 .., ti <= tj); pair (gi, gj) counts when gi < gj < n:
// a diagonal tile leaves out a record's own pairing and keeps equal records at different indices.
// s_acc: a side's keys (values) or adjacency bits (GRAPH), row side 0, column side 1.
template <class Rule, int W, bool GRAPH>
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
    const u16 *q = nullptr;
    if constexpr (Rule::PREFIX) {                            // the row side's s_q behind its planes
        __shared__ u16 s_q[64 * W][RG_TILE];
        if (threadIdx.x < RG_TILE) Rule::template prefix<W>(&s_pl[0][0][0][threadIdx.x], &s_q[0][threadIdx.x]);
        __syncthreads();
        q = &s_q[0][0];
    }
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
        const int v = Rule::template pair<W, GRAPH>(&s_pl[0][0][0][r], &s_pl[1][0][0][lane], Rule::PREFIX ? q + r : q,
                                                    (int)s_len[0][r], lb, t);
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

// One list against another: pair(b, a) for every b of B over a list A, nothing exempted.  A block owns one tile of 64
// records of B, staged once on the reversed (column) side, and streams a range of A's tiles through the plain (row)
// side with the one-list kernel's skewed order: step k pairs column `lane` with row (lane + k) mod 64, a wave taking
// 16 steps of every tile; it is A's records that a rule's s_q belongs to, staged with every tile.  A column's best (a
// key as above, the partner an index into A) or flag lives in LDS for the whole stream and goes out once at the end:
// by atomic maximum, since gridDim.y blocks share a B tile when B alone would not fill the device (block y takes A's
// tiles y * per .. ), or as a byte that is only ever written as 1.  What a block searches depends on the keys it
// read; the maximum, and the smallest partner of equal values, do not.
// FLAGS: the threshold is `above` throughout, a pair ends at its first run beyond it, a flagged column is skipped and
// a tile whose columns are all flagged leaves the stream.
template <class Rule, int W, bool FLAGS>
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
        const u16 *q = nullptr;
        if constexpr (Rule::PREFIX) {
            __shared__ u16 s_q[64 * W][RG_TILE];
            if (threadIdx.x < RG_TILE) Rule::template prefix<W>(&s_pl[0][0][0][threadIdx.x], &s_q[0][threadIdx.x]);
            __syncthreads();
            q = &s_q[0][0];
        }
        const int lb = (int)s_len[1][lane];
        for (u32 k = wave * (RG_TILE * 64 / RG_BLOCK); k < (wave + 1) * (RG_TILE * 64 / RG_BLOCK); ++k) {
            const u32 r = (lane + k) & (RG_TILE - 1);
            const u32 ga = ta * RG_TILE + r;
            if (!(ga < na && gb < nb)) continue;
            const unsigned long long mine = __hip_atomic_load(&s_acc[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (FLAGS && mine) continue;
            const int t = FLAGS ? above : cd_threshold(mine, ga);
            const int v = Rule::template pair<W, FLAGS>(&s_pl[0][0][0][r], &s_pl[1][0][0][lane], Rule::PREFIX ? q + r : q,
                                                        (int)s_len[0][r], lb, t);
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

// the pair launch of either one-list entry: one 64 x 64 tile a block over the upper triangle (values: best; graph:
// bitmap at `above`)
template <class Rule, int W>
static void cd_launch_pairs(hipStream_t s, const CdInput &in, bool graph, u32 n, i32 above, unsigned long long *best,
                            unsigned long long *bitmap) {
    const dim3 grid((unsigned)in.tiles, (unsigned)in.tiles);
    const u32 rowwords = (u32)in.tiles;
    if (graph)
        hipLaunchKernelGGL((cd_pairs_kernel<Rule, W, true>), grid, dim3(RG_BLOCK), 0, s, (const u64 *)in.fwd.p,
                           (const u64 *)in.rev.p, (const u32 *)in.lens.p, n, (u32)in.npad, above, best, bitmap, rowwords);
    else
        hipLaunchKernelGGL((cd_pairs_kernel<Rule, W, false>), grid, dim3(RG_BLOCK), 0, s, (const u64 *)in.fwd.p,
                           (const u64 *)in.rev.p, (const u32 *)in.lens.p, n, (u32)in.npad, above, best, bitmap, rowwords);
}

template <class Rule>
static void cd_pairs(hipStream_t s, const CdInput &in, bool graph, i64 n, i32 above, unsigned long long *best,
                     unsigned long long *bitmap) {
    if (in.W == 1) cd_launch_pairs<Rule, 1>(s, in, graph, (u32)n, above, best, bitmap);
    else if (in.W == 2) cd_launch_pairs<Rule, 2>(s, in, graph, (u32)n, above, best, bitmap);
    else cd_launch_pairs<Rule, 4>(s, in, graph, (u32)n, above, best, bitmap);
}

// the pair launch of either two-list entry: a tile of B a block against the range of A's tiles `per` long that
// blockIdx.y names
template <class Rule, int W>
static void ca_launch(hipStream_t s, dim3 grid, bool flags, const CdInput &A, u32 na, u32 per, const CdInput &B, u32 nb,
                      i32 above, unsigned long long *best, u8 *flag) {
    if (flags)
        hipLaunchKernelGGL((cd_against_kernel<Rule, W, true>), grid, dim3(RG_BLOCK), 0, s, (const u64 *)A.fwd.p,
                           (const u32 *)A.lens.p, na, (u32)A.npad, (u32)A.tiles, per, (const u64 *)B.rev.p,
                           (const u32 *)B.lens.p, nb, (u32)B.npad, above, best, flag);
    else
        hipLaunchKernelGGL((cd_against_kernel<Rule, W, false>), grid, dim3(RG_BLOCK), 0, s, (const u64 *)A.fwd.p,
                           (const u32 *)A.lens.p, na, (u32)A.npad, (u32)A.tiles, per, (const u64 *)B.rev.p,
                           (const u32 *)B.lens.p, nb, (u32)B.npad, above, best, flag);
}

template <class Rule>
static void ca_against(hipStream_t s, dim3 grid, bool flags, const CdInput &A, u32 na, u32 per, const CdInput &B, u32 nb,
                       i32 above, unsigned long long *best, u8 *flag) {
    if (A.W == 1) ca_launch<Rule, 1>(s, grid, flags, A, na, per, B, nb, above, best, flag);
    else if (A.W == 2) ca_launch<Rule, 2>(s, grid, flags, A, na, per, B, nb, above, best, flag);
    else ca_launch<Rule, 4>(s, grid, flags, A, na, per, B, nb, above, best, flag);
}

// What the host side below takes of a rule, so that it exists once: the names in messages, the smallest threshold
// of the graph and flags entries, and the launchers of the two kernels.
struct CdLaunch {
    const char *values_name, *graph_name, *against_name, *flags_name;
    i32 min_above;
    void (*pairs)(hipStream_t s, const CdInput &in, bool graph, i64 n, i32 above, unsigned long long *best,
                  unsigned long long *bitmap);
    void (*against)(hipStream_t s, dim3 grid, bool flags, const CdInput &A, u32 na, u32 per, const CdInput &B, u32 nb,
                    i32 above, unsigned long long *best, u8 *flag);
};

template <class Rule> static constexpr CdLaunch cd_launch() {
    return {Rule::VALUES, Rule::GRAPH, Rule::AGAINST, Rule::FLAGS, Rule::MIN_ABOVE, cd_pairs<Rule>, ca_against<Rule>};
}

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

static void cd_pack(hipStream_t s, const CdInput &in, i64 n) {
    hipLaunchKernelGGL(cd_pack_kernel, dim3((unsigned)div_up(n, 256)), dim3(256), 0, s, (const u8 *)in.d_bytes.p,
                       (const i64 *)in.d_off.p, (u32)n, (u32)in.npad, in.W, in.fwd.p, in.rev.p, in.lens.p);
}

// the values entry of one list: value / partner of every record (host, n entries each)
static int cd_run_values(catchhip_ctx *ctx, const CdLaunch &L, const u8 *bytes, const i64 *off, i64 n, i32 *value,
                         i32 *partner) {
    if (n > CD_MAXN) {
        chip_set_error("%s: %lld records; one call pairs at most %d (%d tiles a side)", L.values_name, (long long)n, CD_MAXN,
                       CD_MAXN / RG_TILE);
        return CATCHHIP_EINVAL;
    }
    CdInput in;
    TRY(cd_check(L.values_name, off, n, &in.W));
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
    cd_pack(s, in, n);
    L.pairs(s, in, false, n, 0, best.p, nullptr);
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

// the graph entry of one list: the conflict graph of `above` as a catchhip_redgraph
static int cd_run_graph(catchhip_ctx *ctx, const CdLaunch &L, const u8 *bytes, const i64 *off, i64 n, i32 above,
                        catchhip_redgraph **out, i64 *nedges) {
    *out = nullptr;
    if (above < L.min_above) {
        chip_set_error("%s: the threshold must be at least %d (%d)", L.graph_name, L.min_above, above);
        return CATCHHIP_EINVAL;
    }
    CdInput in;
    TRY(cd_check(L.graph_name, off, n, &in.W));
    HIP_TRY(hipSetDevice(ctx->device));
    const i64 tiles = div_up(std::max<i64>(n, 1), RG_TILE);
    const double bitmap_bytes = (double)n * (double)tiles * 8.0;
    if (tiles > 65535 || bitmap_bytes > 0.5 * (double)chip_pool_soft_limit()) {
        chip_set_error("%s: %lld records: the adjacency bitmap (%.1f GB) is larger than half of what the "
                       "device-memory cache may hold (%.1f GB)", L.graph_name, (long long)n, bitmap_bytes / 1e9,
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
    cd_pack(s, in, n);
    L.pairs(s, in, true, n, above, nullptr, bitmap.p);
    timer.launch(2);
    TRY(chip_redgraph_from_bitmap(ctx, timer, bitmap.p, tiles, deg.p, G.get()));
    if (nedges) *nedges = G->nedges;
    *out = G.release();
    return 0;
}

#define CA_MAXN ((i64)1 << 30)         // records of either list: the padded count and the tiles stay 32-bit
// Blocks wanted before A's range is split no further: 256 CUs hold 8 blocks of 256 threads each, and blocks end at
// uneven times (the early exits), so the device is level only with several rounds of them -- at 1,563 B tiles and one
// range a CU got 6 or 7 blocks, each as long as the whole stream of A: 1.63 x 10^9 pairs/s for the flags of 100,000
// random 100-mers against 1,000, 2.07 x 10^9 at the 6 ranges this asks for (tools/cross_against_profile.py).
#define CA_FILL 8192

// both two-list entries: checks, both lists packed with one W, the stream of A's tiles; value / partner or flag on
// the host
static int ca_run(catchhip_ctx *ctx, const CdLaunch &L, const u8 *b_bytes, const i64 *b_off, i64 nb, const u8 *a_bytes,
                  const i64 *a_off, i64 na, bool flags, i32 above, i32 *value, i32 *partner, u8 *flag) {
    const char *who = flags ? L.flags_name : L.against_name;
    if (flags && above < L.min_above) {
        chip_set_error("%s: the threshold must be at least %d (%d)", who, L.min_above, above);
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
    cd_pack(s, A, na);
    cd_pack(s, B, nb);
    L.against(s, grid, flags, A, (u32)na, per, B, (u32)nb, above, best.p, d_flag.p);
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
