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
// One list against another (catchhip_cross_against / _flags; include/catchhip_redesign.h): the same planes and the
// same pair function, a tile of B held against the stream of A's tiles.
//
// All of that is in cross_tile.h, for any pair function (duplex.hip has another); this file has cd_pair, the rule that
// names it, and the four entries.
#include "../../include/catchhip_cross.h"
#include "../../include/catchhip_redesign.h"
#include "cross_tile.h"

// run(a, b) where it exceeds t, else some value <= t.  a / rb as cd_match takes them; la / lb are the lengths.
// GRAPH: t + 1 at the first run longer than t.
template <int W, bool GRAPH>
__host__ __device__ static inline int cd_pair(const u64 *a, const u64 *rb, int la, int lb, int t) {
    int best = 0;
    if ((la < lb ? la : lb) <= t) return 0;
    CdSteps steps;
    steps.aim((u32)(t < 63 ? t + 1 : 64));
    for (int c = t; c <= la + lb - 2 - t; ++c) {
        u64 m[W];
        cd_match<W>(a, rb, c, m);
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

// the length rule: nothing staged beside the planes
struct CdLength {
    static constexpr bool PREFIX = false;
    template <int W, bool FIRST>
    __host__ __device__ static __forceinline__ int pair(const u64 *a, const u64 *rb, const u16 *, int la, int lb, int t) {
        return cd_pair<W, FIRST>(a, rb, la, lb, t);
    }
    static constexpr i32 MIN_ABOVE = 1;
    static constexpr const char *VALUES = "cross_dimer", *GRAPH = "cross_dimer_graph", *AGAINST = "cross_against",
                                *FLAGS = "cross_against_flags";
};

// the four entries: cross_tile.h's host side and kernels under the length rule
static constexpr CdLaunch CD_LENGTH = cd_launch<CdLength>();

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
