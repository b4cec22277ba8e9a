// The candidate's L x L table pairs(x, y), 32 cells of an antidiagonal x + y = c at a time, for structure.hip's flag
// kernel and measure.hip's measure_structure_kernel: the bit planes, the walk over an antidiagonal's words, and the
// AND-shifts that find a run of 1-cells inside a word.  Device code only; rule_host.h plans where the planes live.
//
// Bit planes.  The candidate becomes three planes of W = ceil(L / 32) words, bit x of a plane for character x: V (a
// base), B0 and B1 (bits 1 and 2 of the byte: A 00, C 01, T 10, G 11 as B1 B0, so that a base and its complement
// differ in B1 and agree in B0).  Each plane is stored a second time bit-reversed over the 32 W bits, between two
// zero words: cell (x, c - x) needs bit c - x of a plane, which is bit x + (32 W - 1 - c) of the reversed one -- a
// SHIFT of the reversed plane, the same for every x of the antidiagonal.  Word w of the antidiagonal is then
//     m = (B1[w] ^ rB1) & ~(B0[w] ^ rB0) & V[w] & rV,    r* = 32 bits of the reversed plane from bit 32 w + shift,
// one funnel shift per plane over two neighbouring words, of which the lower one is the previous word's upper one.
// Cells outside the table come out 0 by themselves: x >= L has V = 0, y >= L has rV = 0, y < 0 reads the zero word
// behind the reversed plane and y >= 32 W the one in front of it (word indices -1 .. W, shown where they are formed).
// Where the planes live.  They are indexed by the loop counters w and c, the same in every lane but not constants:
// in LDS, or in a global buffer when 64 candidates' planes do not fit the LDS budget.  No array is indexed in
// registers.  A thread's words are contiguous, at a pitch of 6 W + 7 words -- odd, so that the lanes of a wave, which
// read the same word of 64 candidates, are on different banks -- and the three planes are interleaved: word w of V, B0,
// B1 at pl[3 w + 0, 1, 2]; word q of the reversed planes (a zero word, the plane, a zero word: q = 0 .. W + 1) at
// rev[3 q + 0, 1, 2], rev = pl + 3 W.  An iteration's six reads are constant offsets from two pointers that advance by
// three words.  Every lane of a wave walks the same c and w.
#pragma once
#include "internal.h"

__device__ __forceinline__ u32 plane_pitch(u32 W) { return 6u * W + 7u; }

// the planes of the candidate at `row`, from its bytes read as aligned dwords (at most 3 bytes before the row, which
// are the targets' own, and 3 behind it, inside the slack of the byte array)
__device__ __forceinline__ void build_planes(const u8 *row, u32 L, u32 W, u32 *pl) {
    u32 *rev = pl + 3u * W;
    const u32 al = (u32)((uintptr_t)row & 3u);
    const u32 *dw = (const u32 *)(row - al);
    for (u32 p = 0; p < 3u; ++p) { rev[p] = 0; rev[3u * (W + 1u) + p] = 0; }
    u32 cur = dw[0], nd = 1;                                  // cur: the dword that holds byte j
    for (u32 w = 0; w < W; ++w) {
        u32 v = 0, b0 = 0, b1 = 0;
        const u32 cnt = min(32u, L - 32u * w);
        for (u32 t = 0; t < cnt; ++t) {
            const u32 at = al + 32u * w + t;                  // byte offset from dw
            if (at != 0 && (at & 3u) == 0) cur = dw[nd++];                      // nd - 1 = at / 4 <= (al + L - 1) / 4
            const u32 c = (cur >> (8u * (at & 3u))) & 255u;
            const u32 base = (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? 1u : 0u;
            v |= base << t;
            b0 |= ((c >> 1) & 1u) << t;
            b1 |= ((c >> 2) & 1u) << t;
        }
        pl[3u * w] = v;
        pl[3u * w + 1u] = b0;
        pl[3u * w + 2u] = b1;
        // bit z of a reversed plane = bit 32 W - 1 - z of the plane: word W - 1 - w, bits reversed; + 1: the zero word
        rev[3u * (W - w)] = __brev(v);
        rev[3u * (W - w) + 1u] = __brev(b0);
        rev[3u * (W - w) + 2u] = __brev(b1);
    }
}

// the cells of antidiagonal c run from x = antidiagonal_lo to min(L - 1, c); pairs is symmetric, so the callers stop at
// or just past the middle (each says where, and why that is enough)
__device__ __forceinline__ u32 antidiagonal_lo(u32 c, u32 L) { return c > L - 1u ? c - (L - 1u) : 0u; }

// body(w, m) for the words w = lo >> 5 .. upto >> 5 of antidiagonal c, ascending (none when upto >> 5 < lo >> 5), with
// lo = antidiagonal_lo(c, L) and upto <= min(L - 1, c).
// Cell (x, c - x) reads bit 32 W - 1 - c + x of a reversed plane, which is bit x + sh of the stored one (a zero word in
// front: + 32), sh = 32 W + 31 - c.  sh may be "negative" (c up to 64 W - 2): it is kept mod 2^32, and 32 w0 + sh is a
// true bit index again -- 32 w0 >= lo - 31 >= c - L - 30 gives 32 w0 + sh >= 32 W - L + 1 >= 1, and 32 w1 <= upto <= c
// gives 32 w1 + sh <= 32 W + 31: stored words 0 .. W, and W + 1 as the upper word of the last funnel shift.  32 w does
// not touch the low five bits: one o for all w.
template <typename F>
__device__ __forceinline__ void antidiagonal_words(const u32 *pl, u32 W, u32 c, u32 lo, u32 upto, F body) {
    const u32 *rev = pl + 3u * W;
    const u32 sh = 32u * W + 31u - c;
    const u32 o = sh & 31u;
    const u32 w0 = lo >> 5, w1 = upto >> 5;
    const u32 *pf = pl + 3u * w0, *pr = rev + 3u * ((32u * w0 + sh) >> 5);
    u32 lv = pr[0], l0 = pr[1], l1 = pr[2];
    for (u32 w = w0; w <= w1; ++w, pf += 3, pr += 3) {
        const u32 hv = pr[3], h0 = pr[4], h1 = pr[5];                           // reversed word q + 1 <= W + 1
        const u32 rv = __funnelshift_r(lv, hv, o), r0 = __funnelshift_r(l0, h0, o), r1 = __funnelshift_r(l1, h1, o);
        lv = hv; l0 = h0; l1 = h1;
        body(w, (pf[2] ^ r1) & ~(pf[1] ^ r0) & pf[0] & rv);
    }
}

// "Does a word hold `want` consecutive 1-bits": five AND-shifts that grow the run in hand 1 -> want (m & m >> 1 has a
// bit where two cells follow each other, ...; steps 1, 2, 4, 8, 16 at most, a shift of 0 leaves the word as it is:
// want reached), and a mask that is 0 when no word can hold the run (want > 32).
struct RunShifts {
    u32 inword, s0, s1, s2, s3, s4;
    __device__ __forceinline__ void aim(u32 want) {
        inword = want <= 32u ? 0xffffffffu : 0u;
        u32 have = 1, s[5];
        for (int k = 0; k < 5; ++k) {                         // (unrolled: s[] stays in registers)
            s[k] = have < want ? min(have, want - have) & 31u : 0u;
            have += s[k];
        }
        s0 = s[0]; s1 = s[1]; s2 = s[2]; s3 = s[3]; s4 = s[4];
    }
    // bit b of the result <=> bits b .. b + want - 1 of m
    __device__ __forceinline__ u32 inside(u32 m) const {
        u32 x = m & inword;
        x &= x >> s0;
        x &= x >> s1;
        x &= x >> s2;
        x &= x >> s3;
        x &= x >> s4;
        return x;
    }
};
