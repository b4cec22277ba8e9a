// Cross-dimer dG: how firmly two DIFFERENT records of a list hold together, antiparallel, under the unified
// nearest-neighbour parameters (catchhip_cross_duplex and its three siblings; catch_amd/filter/cross_duplex.py has the
// definition).  cross.hip's organisation throughout -- the 64 x 64 tile of pairs, the plain planes of the row side and
// the bit-reversed ones of the column side, one funnel shift per antidiagonal, the rising keys of both sides, a tile
// of B against the stream of A: cross_tile.h's kernels and host side -- under another rule: dx_pair scores the runs
// of an antidiagonal's match word by their bases instead of measuring the longest, from prefix sums (dx_prefix) that a
// block stages beside the row side's planes.
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
        const int d = 64 * W - 1 - c;                        // cd_match's shift
        u64 m[W];
        cd_match<W>(a, rb, c, m);
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

// the dG rule: the row side's prefix sums staged behind its planes
struct DxDuplex {
    static constexpr bool PREFIX = true;
    template <int W> __host__ __device__ static __forceinline__ void prefix(const u64 *a, u16 *q) { dx_prefix<W>(a, q); }
    template <int W, bool FIRST>
    __host__ __device__ static __forceinline__ int pair(const u64 *a, const u64 *rb, const u16 *q, int la, int lb, int t) {
        return dx_pair<W, FIRST>(a, rb, q, la, lb, t);
    }
    static constexpr i32 MIN_ABOVE = 0;
    static constexpr const char *VALUES = "cross_duplex", *GRAPH = "cross_duplex_graph", *AGAINST = "cross_duplex_against",
                                *FLAGS = "cross_duplex_against_flags";
};

// the four entries: cross_tile.h's host side and kernels under the dG rule
static constexpr CdLaunch CD_DUPLEX = cd_launch<DxDuplex>();

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
