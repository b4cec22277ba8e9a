// Base intervals on bitmaps of one bit per base, 64 bases per word: the words and end masks of [a, b), and what the row
// kernels do under them (paint, test, count, mark a difference array).  Device code only; any lane on its own.
// Every helper takes a non-empty interval a < b in global coordinates below 2^32 - 1.
// Tested one by one through catchhip_selftest_spans (tests/test_primitives.py).
#pragma once
#include "internal.h"

// the words of [a, b): nw of them from word w0 on; m0 / m1 = the bits of the first / the last word that lie in the
// interval (one word: both apply to it)
struct Span {
    u32 w0, nw;
    u64 m0, m1;
};
__device__ __forceinline__ Span span_of(u32 a, u32 b) {
    const u32 w0 = a >> 6;
    return Span{w0, ((b - 1) >> 6) - w0 + 1, ~0ull << (a & 63), ~0ull >> (63 - ((b - 1) & 63))};
}
// the bits of word j < nw of the span that lie in the interval
__device__ __forceinline__ u64 span_mask(const Span &sp, u32 j) {
    u64 m = ~0ull;
    if (j == 0) m &= sp.m0;
    if (j == sp.nw - 1) m &= sp.m1;
    return m;
}
// the same from a word's point of view: the bits of the word of bases base .. base + 63 that lie in [a, b); the two
// overlap (a < base + 64, b > base)
__device__ __forceinline__ u64 span_in_word(u64 base, u64 a, u64 b) {
    const u32 lo = a > base ? (u32)(a - base) : 0u;          // < 64
    const u64 hi = b - base;                                 // >= 1
    u64 m = ~0ull << lo;
    if (hi < 64) m &= ~0ull >> (64 - (u32)hi);
    return m;
}

// bm |= [a, b).  Rows of several sets overlap and most words are complete already: the test spares the atomic
__device__ __forceinline__ void span_paint(unsigned long long *__restrict__ bm, u32 a, u32 b) {
    const Span sp = span_of(a, b);
    for (u32 j = 0; j < sp.nw; ++j) {
        const u64 m = span_mask(sp, j);
        if ((bm[sp.w0 + j] & m) != m) atomicOr(&bm[sp.w0 + j], m);
    }
}
// is every bit of [a, b) set in bm?  Leaves at the first word that has a clear one
__device__ __forceinline__ bool span_all_set(const unsigned long long *__restrict__ bm, u32 a, u32 b) {
    const Span sp = span_of(a, b);
    for (u32 j = 0; j < sp.nw; ++j) {
        const u64 m = span_mask(sp, j);
        if ((bm[sp.w0 + j] & m) != m) return false;
    }
    return true;
}
// the set bits of bm under word j < nw of the span (for a loop strided over a wavefront or a workgroup) ...
__device__ __forceinline__ u32 span_popc_word(const unsigned long long *__restrict__ bm, const Span &sp, u32 j) {
    return (u32)__popcll(bm[sp.w0 + j] & span_mask(sp, j));
}
// ... and under all of [a, b), by one lane
__device__ __forceinline__ u32 span_popc(const unsigned long long *__restrict__ bm, u32 a, u32 b) {
    const Span sp = span_of(a, b);
    u32 c = 0;
    for (u32 j = 0; j < sp.nw; ++j) c += span_popc_word(bm, sp, j);
    return c;
}

// [a, b) on a difference array (u32, wrapping; total + 1 entries at least: a row may end at total): after an exclusive
// scan, d[x + 1] = the intervals over base x.  Integer atomics: the result does not depend on the order of the marks
__device__ __forceinline__ void span_mark_diff(u32 *__restrict__ d, u32 a, u32 b) {
    atomicAdd(&d[a], 1u);
    atomicAdd(&d[b], 0xffffffffu);
}
