/*
 * catchhip_redesign.h -- the entry points of libcatchhip.so behind the
 * cross-dimer redesign (SetCoverFilter(..., max_cross_dimer=X)), beside
 * catchhip.h (whose types, error codes and conventions hold here) and
 * catchhip_cross.h (whose run(s, t) is the one meant here): one list of records
 * against another, and a row table without some of its sets.  Not in the
 * reference.
 *
 * For a record b and a list A of na records,
 *   cross_against(b, A) = max over a in A of run(b, a); 0 for an empty A.  A
 *                         member of A equal to b is a partner like any other
 *                         (the value is then run(b, b)): nothing is exempted.
 *   its partner         = the smallest index into A that reaches the value; -1
 *                         if the value is 0.
 *   conflicts_with(b, A, X) iff cross_against(b, A) > X.
 * Both pair entries take two lists in catchhip_cross_dimer's form: nb records
 * at b_bytes / b_off[nb + 1] and na at a_bytes / a_off[na + 1], any bytes,
 * 0 .. 256 characters each and of any mix of lengths; the word count of the bit
 * planes is chosen over both lists (CATCHHIP_EINVAL names the limit for a
 * longer record).  Either list may be empty (value 0, partner -1, flag 0
 * everywhere; the other list's pointers may then be NULL as well).  More than
 * 2^30 records in a list are refused with CATCHHIP_EINVAL.  All na * nb pairs
 * are evaluated on the device (csrc/cross.hip), exactly; the results are the
 * same bytes on every run.
 */
#ifndef CATCHHIP_REDESIGN_H
#define CATCHHIP_REDESIGN_H

#include "catchhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* value[i] = cross_against(b_i, A), partner[i] = its partner, an index into A
 * (host, nb entries each). */
int catchhip_cross_against(catchhip_ctx *ctx, const uint8_t *b_bytes,
                           const int64_t *b_off, int64_t nb,
                           const uint8_t *a_bytes, const int64_t *a_off,
                           int64_t na, int32_t *value, int32_t *partner);
/* flag[i] = 1 iff conflicts_with(b_i, A, above), else 0 (host, nb bytes;
 * above >= 1, else CATCHHIP_EINVAL).  The pair kernel leaves a pair at its
 * first run beyond `above`, a record of B once it is flagged and a tile of 64
 * of them once all are. */
int catchhip_cross_against_flags(catchhip_ctx *ctx, const uint8_t *b_bytes,
                                 const int64_t *b_off, int64_t nb,
                                 const uint8_t *a_bytes, const int64_t *a_off,
                                 int64_t na, int32_t above, uint8_t *flag);
/* *out = the rows of `rows` (a table in the solver's form, as
 * catchhip_rows_subtract takes it) whose set has drop[set] == 0 (host,
 * num_sets bytes): order, universes and set ids kept, gain0 carried for the
 * surviving sets (0 for the others), the longest row exact -- a table for
 * catchhip_setcover_greedy, catchhip_rows_subtract and
 * catchhip_rows_below_depth as it is.  *nrows (may be NULL) = its rows.
 * CATCHHIP_EINVAL: what catchhip_rows_subtract refuses in its first table
 * (deferred rows, the direct form, group numbers, the limits of 32-bit
 * coordinates), and a row whose set id is not below num_sets. */
int catchhip_rows_drop_sets(catchhip_ctx *ctx, const catchhip_rows *rows,
                            int64_t num_sets, const uint8_t *drop,
                            catchhip_rows **out, int64_t *nrows);

#ifdef __cplusplus
}
#endif
#endif /* CATCHHIP_REDESIGN_H */
