/*
 * catchhip_cross.h -- the cross-dimer entry points of libcatchhip.so, beside
 * catchhip.h (whose types, error codes and conventions hold here): how far two
 * DIFFERENT records of a list pair with each other.  Not in the reference.
 *
 * A record is a string of bytes as they are: only 'A', 'C', 'G', 'T' are
 * bases; 'N', lower case and every other byte pair with nothing.  For records
 * s and t, pairs(x, y) holds iff s[x] and t[y] are bases and t[y] is the
 * Watson-Crick complement of s[x], and
 *   run(s, t)  = the largest n for which there are a, b with
 *                pairs(a + k, b - k) for k in 0 .. n - 1, every index inside
 *                its record; 0 if there is none.  run(s, t) = run(t, s) = the
 *                longest common substring of s and revcomp(t) over bases.
 *   cross(i)   = max over j != i of run(s_i, s_j); 0 for a list of one.  An
 *                equal record at another index is a partner like any other;
 *                the record itself is not (that is `dimer`,
 *                catchhip_candidates_measure).
 *   partner(i) = the smallest j != i with run(s_i, s_j) = cross(i); -1 if
 *                cross(i) = 0.
 * Both entries take catchhip_redundancy_graph's input: n records at bytes /
 * off[n + 1], any bytes, 0 .. 256 characters each and of any mix of lengths
 * (CATCHHIP_EINVAL names the limit otherwise).  All n (n - 1) / 2 pairs are
 * evaluated on the device (csrc/cross.hip), exactly; the results are the same
 * bytes on every run.
 */
#ifndef CATCHHIP_CROSS_H
#define CATCHHIP_CROSS_H

#include "catchhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* value[i] = cross(i), partner[i] = partner(i) (host, n entries each).  More
 * than 1,048,576 records (16,384 tiles of 64 a side) are refused with
 * CATCHHIP_EINVAL. */
int catchhip_cross_dimer(catchhip_ctx *ctx, const uint8_t *bytes,
                         const int64_t *off, int64_t n, int32_t *value,
                         int32_t *partner);
/* The conflict graph of a threshold: i and j (i != j) are neighbours iff
 * run(s_i, s_j) > above (above >= 1, else CATCHHIP_EINVAL), as an ordinary
 * catchhip_redgraph -- symmetric, no self loops, every neighbour list
 * ascending, *nedges (may be NULL) two per conflicting pair -- for
 * catchhip_redundancy_fetch / _naive / _rows / _destroy.  The pair kernel
 * leaves a pair at its first run beyond `above`.  The size limit is
 * catchhip_redundancy_graph's (the adjacency bitmap). */
int catchhip_cross_dimer_graph(catchhip_ctx *ctx, const uint8_t *bytes,
                               const int64_t *off, int64_t n, int32_t above,
                               catchhip_redgraph **out, int64_t *nedges);

#ifdef __cplusplus
}
#endif
#endif /* CATCHHIP_CROSS_H */
