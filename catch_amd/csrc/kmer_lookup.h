// One position's look-up in a catchhip_kmer_index, for background.hip's flag kernels and measure.hip's "hits" family
// (background.hip's head says what the index holds).  fwd and rc are the rolled codes of the position's k-mer and of
// its reverse complement; the caller has checked that the k-mer is valid.  Both forms return 1 for a hit, 0 otherwise.
#pragma once
#include "internal.h"

// ---- exact: canonical(w) is among the codes ----------------------------------------------------------------------
// dir[p] and dir[p + 1] (one gather of two neighbouring words), then the bucket -- halved while it is longer than 4,
// then compared one by one.
__device__ __forceinline__ u32 kmer_lookup_exact(u64 fwd, u64 rc, const u64 *__restrict__ codes,
                                                 const u32 *__restrict__ dir, u32 dir_shift) {
    const u64 canon = fwd < rc ? fwd : rc;
    const u32 b = (u32)(canon >> dir_shift);
    u32 lo = dir[b], hi = dir[b + 1u];
    while (hi - lo > 4u) {                                    // (canon, if it is there at all, stays inside [lo, hi))
        const u32 mid = (lo + hi) >> 1;
        if (codes[mid] <= canon) lo = mid; else hi = mid;
    }
    u32 hit = 0;
    for (u32 t = lo; t < hi; ++t) hit |= codes[t] == canon ? 1u : 0u;
    return hit;
}

// ---- tolerant: some code lies within M mismatches of fwd or of rc --------------------------------------------------
// The M + 1 views of a tolerant index as the kernels receive them (by value, in the kernel arguments).  View b holds
// every code rotated left by rot[b] = 2 s_b bits inside its 2K bits (rot[0] = 0), sorted, and a directory over the top
// 2K - dir_shift[b] bits, which are never more than block b's: every code that agrees with a query in block b lies in
// the one bucket the rotated query's top bits select.
struct KmerViews {
    const u64 *codes[3];
    const u32 *dir[3];
    u32 dir_shift[3];
    u32 rot[3];
};

static inline KmerViews kmer_views(const catchhip_kmer_index *X) {
    KmerViews v = {};
    const u32 bits = 2u * (u32)X->k;
    v.codes[0] = X->codes;
    v.dir[0] = X->dir;
    v.dir_shift[0] = bits - X->P;
    for (i32 b = 1; b <= X->mismatches; ++b) {
        v.codes[b] = X->view_codes[b - 1];
        v.dir[b] = X->view_dir[b - 1];
        v.dir_shift[b] = bits - X->view_P[b - 1];
        v.rot[b] = 2u * X->view_start[b - 1];
    }
    return v;
}

// characters in which two codes differ (rotated alike or not at all)
__device__ __forceinline__ u32 kmer_distance(u64 x, u64 c) {
    const u64 d = x ^ c;
    return (u32)__popcll((d | (d >> 1)) & 0x5555555555555555ull);
}

// Two k-mers within M mismatches agree exactly in one of the M + 1 blocks, and d(w, revcomp(v)) = d(revcomp(w), v):
// fwd and rc each go into every view, 2 (M + 1) buckets, and whatever a bucket holds within distance M is a hit,
// whether or not it agrees in the block.  The 2 (M + 1) directory gathers are issued before the first bucket is read,
// then the first entry of every bucket, so that their latencies overlap; what is left of a bucket is walked entry by
// entry, to the first hit.  A palindrome (fwd == rc) looks up one word.
template <int M>
__device__ __forceinline__ u32 kmer_lookup_tolerant(u64 fwd, u64 rc, u64 mask, u32 two_k, const KmerViews &v) {
    constexpr int NQ = 2 * (M + 1);
    u64 q[NQ], first[NQ];
    u32 lo[NQ], hi[NQ];
    const bool both = fwd != rc;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int b = i >> 1;
        const u64 x = (i & 1) ? rc : fwd;
        // (view 0 is not rotated; above it 0 < rot < 2K <= 64, so neither shift reaches the word's width)
        q[i] = b == 0 ? x : ((x << v.rot[b]) | (x >> (two_k - v.rot[b]))) & mask;
        const u32 p = (u32)(q[i] >> v.dir_shift[b]);
        lo[i] = v.dir[b][p];
        hi[i] = ((i & 1) && !both) ? lo[i] : v.dir[b][p + 1u];
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i)                              // (~q differs from q in every character)
        first[i] = lo[i] < hi[i] ? v.codes[i >> 1][lo[i]] : ~q[i];
    u32 hit = 0;
#pragma unroll
    for (int i = 0; i < NQ; ++i) hit |= kmer_distance(q[i], first[i]) <= (u32)M ? 1u : 0u;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const u64 *__restrict__ codes = v.codes[i >> 1];
        for (u32 t = lo[i] + 1u; !hit && t < hi[i]; ++t) hit = kmer_distance(q[i], codes[t]) <= (u32)M ? 1u : 0u;
    }
    return hit;
}
