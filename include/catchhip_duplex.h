/*
 * catchhip_duplex.h -- the cross-dimer dG entry points of libcatchhip.so,
 * beside catchhip_cross.h and catchhip_redesign.h (whose records, pairs(x, y),
 * shapes, limits and error codes hold here): how FIRMLY two different records
 * pair with each other, instead of over how many bases.  Not in the reference.
 *
 * dg(d) is the unified nearest-neighbour free energy (SantaLucia 1998, 37
 * degrees C, 1 M NaCl) of the dinucleotide d read 5'->3' on one strand, in
 * hundredths of a kcal/mol:
 *   AA TT -100   AT -88   TA -58   CA TG -145   GT AC -144   CT AG -128
 *   GA TC -130   CG -217  GC -224  GG CC -184
 * and term(c) = +98 for G or C, +103 for A or T.  A stretch of records s, t is
 * (a, b, n), n >= 2, with pairs(a + k, b - k) for k in 0 .. n - 1, and
 *   stab(a, b, n) = -(sum over k in 0 .. n - 2 of dg(s[a+k] s[a+k+1])
 *                     + term(s[a]) + term(s[a+n-1]))
 *   duplex(s, t)  = the maximum of stab over all stretches; 0 if that is
 *                   negative or there is none.  duplex(s, t) = duplex(t, s).
 *   dcross(i)     = max over j != i of duplex(s_i, s_j); 0 for a list of one.
 *                   An equal record at another index is a partner.
 *   dpartner(i)   = the smallest j != i that reaches dcross(i); -1 at 0.
 *   duplex_against(b, A) = max over a in A of duplex(b, a), nothing exempted,
 *                   and its partner the smallest index into A that reaches it.
 * Records hold 0 .. 256 characters in any mix of lengths (CATCHHIP_EINVAL names
 * the limit otherwise).  Every pair is evaluated on the device
 * (csrc/duplex.hip), exactly; the results are the same bytes on every run.
 */
#ifndef CATCHHIP_DUPLEX_H
#define CATCHHIP_DUPLEX_H

#include "catchhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* value[i] = dcross(i), partner[i] = dpartner(i) (host, n entries each).  More
 * than 1,048,576 records are refused with CATCHHIP_EINVAL. */
int catchhip_cross_duplex(catchhip_ctx *ctx, const uint8_t *bytes,
                          const int64_t *off, int64_t n, int32_t *value,
                          int32_t *partner);
/* The conflict graph of a threshold: i and j (i != j) are neighbours iff
 * duplex(s_i, s_j) > above (above >= 0, else CATCHHIP_EINVAL), as an ordinary
 * catchhip_redgraph for catchhip_redundancy_fetch / _naive / _rows /
 * _destroy, as catchhip_cross_dimer_graph builds it and with its size limit
 * (the adjacency bitmap). */
int catchhip_cross_duplex_graph(catchhip_ctx *ctx, const uint8_t *bytes,
                                const int64_t *off, int64_t n, int32_t above,
                                catchhip_redgraph **out, int64_t *nedges);
/* value[i] = duplex_against(b_i, A), partner[i] = its partner, an index into A
 * (host, nb entries each); the lists as catchhip_cross_against takes them. */
int catchhip_cross_duplex_against(catchhip_ctx *ctx, const uint8_t *b_bytes,
                                  const int64_t *b_off, int64_t nb,
                                  const uint8_t *a_bytes, const int64_t *a_off,
                                  int64_t na, int32_t *value, int32_t *partner);
/* flag[i] = 1 iff duplex_against(b_i, A) > above, else 0 (host, nb bytes;
 * above >= 0, else CATCHHIP_EINVAL), with catchhip_cross_against_flags' early
 * exits. */
int catchhip_cross_duplex_against_flags(catchhip_ctx *ctx,
                                        const uint8_t *b_bytes,
                                        const int64_t *b_off, int64_t nb,
                                        const uint8_t *a_bytes,
                                        const int64_t *a_off, int64_t na,
                                        int32_t above, uint8_t *flag);

#ifdef __cplusplus
}
#endif
#endif /* CATCHHIP_DUPLEX_H */
