// Cross-dimer dG: how firmly two DIFFERENT records of a list hold together, antiparallel, under the unified
// nearest-neighbour parameters (catchhip_cross_duplex and its three siblings; catch_amd/filter/cross_duplex.py has the
// definition).  cross.hip's organisation throughout -- the 64 x 64 tile of pairs, the plain planes of the row side and
// the bit-reversed ones of the column side, one funnel shift per antidiagonal, the rising keys of both sides, a tile
// of B against the stream of A -- with another pair function: dx_pair scores the runs of an antidiagonal's match word
// by their bases instead of measuring the longest.
//
// Stability.  A stretch of n >= 2 pairs that starts at row position x has
//     stab = Q[x + n - 1] - Q[x] - term(x) - term(x + n - 1),
// Q[x] = the sum of -dg over the row record's dinucleotides (k, k + 1), k < x, in hundredths of a kcal/mol, a
// dinucleotide with a non-base counting 0 (inside a run there is none), term = 103 for A / T and 98 for C / G.  The
// ROW record alone decides: the column's bases are the complements.  Q is at most 224 * 255 = 57,120, an unsigned
// 16-bit word; a tile's row side stages it beside the planes as s_q[64 W positions][64 records], computed from the
// staged planes by one thread per record (32 KB at W = 4 beside the planes' 24 KB).  Plane B0 is 1 exactly for C and
// G and gives the terminals.
//
// Search.  One more pair adds at least 58 and moves a terminal by at most 5, so the firmest stretch is a MAXIMAL run
// of the match word, and a run of n pairs has stab <= 224 (n - 1) - 196: against a threshold t no run of at most
// L(t) = (t + 196) / 224 + 1 pairs matters.  So the AND-shift search is aimed at L + 1 (at most 64): afterwards bit b
// of m says that L + 1 pairs start at b, each maximal run of n >= L + 1 pairs has become a run of n - L bits with the
// same head, the k-th head bit (m & ~(m << 1)) belongs to the k-th tail bit (m & ~(m >> 1)), and head and tail + L
// are the ends whose Q and terminals give the run's stab.  An antidiagonal of at most L cells is never looked at.
// For d < 0 the row's planes are the shifted ones: bit b is row position b - d.
//
// Values reach 57,120 - 196, so the keys (value << 32) | (0xFFFFFFFF - partner) hold them, and cd_threshold's rule is
// the length kernel's.  The graph and flags entries fix the threshold at `above` >= 0 and leave a pair at its first
// run beyond it.
#include "../../include/catchhip_duplex.h"
#include "cross_tile.h"

// -dg of the dinucleotide (first, second) in the planes' code B0 | B1 << 1: A 0, C 1, T 2, G 3 (SantaLucia 1998,
// unified, 37 degrees C, 1 M NaCl; hundredths of a kcal/mol, one byte each, entry first * 4 + second)
//   AA 100  AC 144  AT  88  AG 128  CA 145  CC 184  CT 128  CG 217
//   TA  58  TC 130  TT 100  TG 145  GA 130  GC 224  GT 144  GG 184
__host__ __device__ __forceinline__ u32 dx_stack(u32 first, u32 second) {
    const u32 i = first * 4 + second;
    const u64 half = i < 8 ? 0xD980B89180589064ull : 0xB890E0829164823Aull;
    return (u32)(half >> ((i & 7u) * 8)) & 255u;
}

// q[x * RG_TILE] = Q[x] for the 64 W positions of the record whose plain planes a points at (a tile's layout, as
// dx_pair takes it; word W of a plane is zero)
template <int W> __host__ __device__ static inline void dx_prefix(const u64 *a, u16 *q) {
    u32 acc = 0;
    for (int w = 0; w < W; ++w) {
        const u64 v = a[(size_t)(0 * 2 * W + w) * RG_TILE], b0 = a[(size_t)(1 * 2 * W + w) * RG_TILE],
                  b1 = a[(size_t)(2 * 2 * W + w) * RG_TILE];
        // the same planes one position on
        const u64 v1 = (v >> 1) | (a[(size_t)(0 * 2 * W + w + 1) * RG_TILE] << 63),
                  b01 = (b0 >> 1) | (a[(size_t)(1 * 2 * W + w + 1) * RG_TILE] << 63),
                  b11 = (b1 >> 1) | (a[(size_t)(2 * 2 * W + w + 1) * RG_TILE] << 63);
        const u64 both = v & v1;
        for (u32 i = 0; i < 64; ++i) {
            q[(size_t)(w * 64 + i) * RG_TILE] = (u16)acc;
            const u32 first = (u32)((b0 >> i) & 1u) | ((u32)((b1 >> i) & 1u) << 1);
            const u32 second = (u32)((b01 >> i) & 1u) | ((u32)((b11 >> i) & 1u) << 1);
            acc += ((both >> i) & 1u) ? dx_stack(first, second) : 0u;
        }
    }
}

// The match word of antidiagonal c = 64 W - 1 - d, as cd_pair builds it.  a points at word 0 of plane V of the row
// record's plain planes, rb at the same of the column record's reversed planes, both in a tile's layout
// [plane][2 W words][RG_TILE] with words W .. 2 W - 1 zero (a shifted read never leaves the array).  For d >= 0 bit x
// of m is cell (x, c - x), for d < 0 bit x is cell (x - d, c - x + d): the row's planes are then the shifted ones.
template <int W>
__host__ __device__ __forceinline__ void dx_match(const u64 *a, const u64 *rb, int d, u64 (&m)[W]) {
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

// runs of at most this many pairs cannot exceed t
__host__ __device__ __forceinline__ int dx_short(int t) { return (t + 196) / 224 + 1; }

// duplex(a, b) where it exceeds t >= 0, else some value <= t.  a / rb / la / lb as cd_pair takes them, q the row
// record's prefix sums (dx_prefix).  GRAPH: the first stab beyond t.
template <int W, bool GRAPH>
__host__ __device__ static inline int dx_pair(const u64 *a, const u64 *rb, const u16 *q, int la, int lb, int t) {
    int best = 0;
    int L = dx_short(t);
    if ((la < lb ? la : lb) <= L) return 0;
    CdSteps steps;
    steps.aim((u32)(L < 63 ? L + 1 : 64));
    for (int c = L; c <= la + lb - 2 - L; ++c) {
        const int d = 64 * W - 1 - c;                        // |d| <= 64 W - 1: la + lb - 2 <= 128 W - 2
        u64 m[W];
        dx_match<W>(a, rb, d, m);
        steps.inside<W>(m);
        if (!cd_any<W>(m)) continue;
        // bit b of m: steps.want pairs start at b.  Heads of its runs, and their tails: the k-th of each are one run
        const int x0 = d < 0 ? -d : 0;                       // bit b is row position b + x0
        const int more = (int)steps.want - 1 + x0;
        u64 hd[W], tl[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const u64 below = w ? m[w - 1] >> 63 : 0ull, above = w + 1 < W ? m[w + 1] << 63 : 0ull;
            hd[w] = m[w] & ~((m[w] << 1) | below);
            tl[w] = m[w] & ~((m[w] >> 1) | above);
        }
        bool rose = false;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            while (hd[w]) {
                const int xa = w * 64 + __builtin_ctzll(hd[w]) + x0;
                hd[w] &= hd[w] - 1;
                int xz = -1;                                 // the first tail left: this head's
#pragma unroll
                for (int u = 0; u < W; ++u)
                    if (xz < 0 && tl[u]) {
                        xz = u * 64 + __builtin_ctzll(tl[u]) + more;
                        tl[u] &= tl[u] - 1;
                    }
                // (xa < xz <= 64 W - 1: a match bit stands only where both records have a base)
                const u32 gc = (u32)((a[(size_t)(1 * 2 * W + (xa >> 6)) * RG_TILE] >> (xa & 63)) & 1u) +
                               (u32)((a[(size_t)(1 * 2 * W + (xz >> 6)) * RG_TILE] >> (xz & 63)) & 1u);
                const int v = (int)q[(size_t)xz * RG_TILE] - (int)q[(size_t)xa * RG_TILE] - 206 + 5 * (int)gc;
                if (v > t) {
                    if (GRAPH) return v;
                    best = t = v;
                    rose = true;
                }
            }
        }
        if (rose) {                                          // (m was searched with the old aim: only now)
            L = dx_short(t);
            steps.aim((u32)(L < 63 ? L + 1 : 64));
        }
    }
    return best;
}

// cd_pairs_kernel with dx_pair: the row side's prefix sums staged behind its planes
template <int W, bool GRAPH>
__global__ void __launch_bounds__(RG_BLOCK)
dx_pairs_kernel(const u64 *__restrict__ fwd, const u64 *__restrict__ rev, const u32 *__restrict__ lens, u32 n, u32 npad,
                i32 above, unsigned long long *best, unsigned long long *bitmap, u32 rowwords) {
    const u32 ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    __shared__ u64 s_pl[2][3][2 * W][RG_TILE];
    __shared__ u16 s_q[64 * W][RG_TILE];
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
    if (threadIdx.x < RG_TILE) dx_prefix<W>(&s_pl[0][0][0][threadIdx.x], &s_q[0][threadIdx.x]);
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
        const int v = dx_pair<W, GRAPH>(&s_pl[0][0][0][r], &s_pl[1][0][0][lane], &s_q[0][r], (int)s_len[0][r], lb, t);
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
static void dx_launch_pairs(hipStream_t s, const CdInput &in, bool graph, u32 n, i32 above, unsigned long long *best,
                            unsigned long long *bitmap) {
    const dim3 grid((unsigned)in.tiles, (unsigned)in.tiles);
    const u32 rowwords = (u32)in.tiles;
    if (graph)
        hipLaunchKernelGGL((dx_pairs_kernel<W, true>), grid, dim3(RG_BLOCK), 0, s, (const u64 *)in.fwd.p, (const u64 *)in.rev.p,
                           (const u32 *)in.lens.p, n, (u32)in.npad, above, best, bitmap, rowwords);
    else
        hipLaunchKernelGGL((dx_pairs_kernel<W, false>), grid, dim3(RG_BLOCK), 0, s, (const u64 *)in.fwd.p, (const u64 *)in.rev.p,
                           (const u32 *)in.lens.p, n, (u32)in.npad, above, best, bitmap, rowwords);
}

static void dx_pairs(hipStream_t s, const CdInput &in, bool graph, i64 n, i32 above, unsigned long long *best,
                     unsigned long long *bitmap) {
    if (in.W == 1) dx_launch_pairs<1>(s, in, graph, (u32)n, above, best, bitmap);
    else if (in.W == 2) dx_launch_pairs<2>(s, in, graph, (u32)n, above, best, bitmap);
    else dx_launch_pairs<4>(s, in, graph, (u32)n, above, best, bitmap);
}

// cd_against_kernel with dx_pair: the tile of B on the column side for the whole stream, every tile of A staged on the
// row side with its prefix sums (it is A's records that score a run)
template <int W, bool FLAGS>
__global__ void __launch_bounds__(RG_BLOCK)
dx_against_kernel(const u64 *__restrict__ a_fwd, const u32 *__restrict__ a_lens, u32 na, u32 a_npad, u32 a_tiles, u32 per,
                  const u64 *__restrict__ b_rev, const u32 *__restrict__ b_lens, u32 nb, u32 b_npad, i32 above,
                  unsigned long long *best, u8 *flag) {
    const u32 tb = blockIdx.x;
    const u32 t_lo = blockIdx.y * per, t_hi = t_lo + per < a_tiles ? t_lo + per : a_tiles;
    if (t_lo >= t_hi) return;
    __shared__ u64 s_pl[2][3][2 * W][RG_TILE];
    __shared__ u16 s_q[64 * W][RG_TILE];
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
        if (threadIdx.x < RG_TILE) dx_prefix<W>(&s_pl[0][0][0][threadIdx.x], &s_q[0][threadIdx.x]);
        __syncthreads();
        const int lb = (int)s_len[1][lane];
        for (u32 k = wave * (RG_TILE * 64 / RG_BLOCK); k < (wave + 1) * (RG_TILE * 64 / RG_BLOCK); ++k) {
            const u32 r = (lane + k) & (RG_TILE - 1);
            const u32 ga = ta * RG_TILE + r;
            if (!(ga < na && gb < nb)) continue;
            const unsigned long long mine = __hip_atomic_load(&s_acc[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (FLAGS && mine) continue;
            const int t = FLAGS ? above : cd_threshold(mine, ga);
            const int v = dx_pair<W, FLAGS>(&s_pl[0][0][0][r], &s_pl[1][0][0][lane], &s_q[0][r], (int)s_len[0][r], lb, t);
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
static void dx_launch_against(hipStream_t s, dim3 grid, bool flags, const CdInput &A, u32 na, u32 per, const CdInput &B,
                              u32 nb, i32 above, unsigned long long *best, u8 *flag) {
    if (flags)
        hipLaunchKernelGGL((dx_against_kernel<W, true>), grid, dim3(RG_BLOCK), 0, s, (const u64 *)A.fwd.p, (const u32 *)A.lens.p,
                           na, (u32)A.npad, (u32)A.tiles, per, (const u64 *)B.rev.p, (const u32 *)B.lens.p, nb, (u32)B.npad,
                           above, best, flag);
    else
        hipLaunchKernelGGL((dx_against_kernel<W, false>), grid, dim3(RG_BLOCK), 0, s, (const u64 *)A.fwd.p, (const u32 *)A.lens.p,
                           na, (u32)A.npad, (u32)A.tiles, per, (const u64 *)B.rev.p, (const u32 *)B.lens.p, nb, (u32)B.npad,
                           above, best, flag);
}

static void dx_against(hipStream_t s, dim3 grid, bool flags, const CdInput &A, u32 na, u32 per, const CdInput &B, u32 nb,
                       i32 above, unsigned long long *best, u8 *flag) {
    if (A.W == 1) dx_launch_against<1>(s, grid, flags, A, na, per, B, nb, above, best, flag);
    else if (A.W == 2) dx_launch_against<2>(s, grid, flags, A, na, per, B, nb, above, best, flag);
    else dx_launch_against<4>(s, grid, flags, A, na, per, B, nb, above, best, flag);
}

// the four entries: cross_tile.h's host side over this file's kernels
static const CdLaunch CD_DUPLEX = {"cross_duplex", "cross_duplex_graph", "cross_duplex_against", "cross_duplex_against_flags",
                                   0, dx_pairs, dx_against};

extern "C" int catchhip_cross_duplex(catchhip_ctx *ctx, const u8 *bytes, const i64 *off, i64 n, i32 *value, i32 *partner) {
    ARG_CHECK(ctx && off && n >= 0 && (n == 0 || (bytes && value && partner)));
    return cd_run_values(ctx, CD_DUPLEX, bytes, off, n, value, partner);
}

extern "C" int catchhip_cross_duplex_graph(catchhip_ctx *ctx, const u8 *bytes, const i64 *off, i64 n, i32 above,
                                           catchhip_redgraph **out, i64 *nedges) {
    ARG_CHECK(ctx && out && off && n >= 0 && (n == 0 || bytes));
    return cd_run_graph(ctx, CD_DUPLEX, bytes, off, n, above, out, nedges);
}

extern "C" int catchhip_cross_duplex_against(catchhip_ctx *ctx, const u8 *b_bytes, const i64 *b_off, i64 nb,
                                             const u8 *a_bytes, const i64 *a_off, i64 na, i32 *value, i32 *partner) {
    ARG_CHECK(ctx && na >= 0 && nb >= 0 && (nb == 0 || (b_bytes && b_off && value && partner)) &&
              (na == 0 || (a_bytes && a_off)));
    return ca_run(ctx, CD_DUPLEX, b_bytes, b_off, nb, a_bytes, a_off, na, false, 0, value, partner, nullptr);
}

extern "C" int catchhip_cross_duplex_against_flags(catchhip_ctx *ctx, const u8 *b_bytes, const i64 *b_off, i64 nb,
                                                   const u8 *a_bytes, const i64 *a_off, i64 na, i32 above, u8 *flag) {
    ARG_CHECK(ctx && na >= 0 && nb >= 0 && (nb == 0 || (b_bytes && b_off && flag)) && (na == 0 || (a_bytes && a_off)));
    return ca_run(ctx, CD_DUPLEX, b_bytes, b_off, nb, a_bytes, a_off, na, true, above, nullptr, nullptr, flag);
}
