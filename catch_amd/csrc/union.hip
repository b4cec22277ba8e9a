// The union of two row tables, set by set (catchhip_rows_union): the cover sets of SetCoverFilter(either_strand=True),
// where candidate i covers what its own string or its reverse complement hybridises to.
//
// Both tables are in the solver's form: sorted by (set, universe, start), the rows of a (set, universe) disjoint and
// non-touching.  Universes lie side by side in global coordinates, so a table is sorted by the 64-bit key (set, gs),
// and -- its rows being disjoint -- by (set, ge) as well.  Inside one table nothing overlaps or touches, so only a row
// of the OTHER table can absorb a row, and no sort and no merge path are needed:
//
//   union_flag_kernel   a lane per input row r (the blocks of `a` first, then those of `b`).  r is the HEAD of a union
//                       interval iff no row q of the other table, same set and universe, has q.start < r.start <= q.end,
//                       and its TAIL iff no such q has q.start <= r.end < q.end (equal starts: a's row is the head; equal
//                       ends: a's row is the tail).  The other table being in normal form, one row can be that q: the last
//                       one whose (set, gs) lies below r's for the head, the first one whose (set, ge) lies above r's for
//                       the tail -- two binary searches.  Their positions are kept beside the flags.  A wavefront's
//                       rows are consecutive, so its first and last row search the whole table and the 62 between
//                       them only the rows between those two answers.
//   two exclusive scans of the head flags and of the tail flags, each over a's rows followed by b's
//   read-back of the scans' last entries: the number of heads (= rows of the result) and of tails
//   union_emit_kernel   the output index of a head = the heads before it in its own table + the heads of the other
//                       table below its key (the scan at the position the search left): it writes set, universe and
//                       start.  A tail's index is the same over (set, ge): it writes the end.  Inside a set the union
//                       intervals are ordered and disjoint, so the k-th head and the k-th tail are one output row.
//   union_sum_kernel    one pass over the output: gain0[set] += length (runs of one set inside a wavefront summed first)
//                       and the longest row.
//
// Rows of different universes that touch in global coordinates (the last base of universe u, the first of u + 1) do not
// merge: every absorption test compares the universes.  Integer arithmetic only and the atomics commute: the result
// does not depend on the launch geometry.  Scratch: 16 bytes per input row.
#include <algorithm>

#include "rows_host.h"
#include "wave.h"

typedef unsigned long long ull;

#define UN_FLAG 0x80000000u   // bit 31 of a kept search position: the row is a head / a tail (positions stay below 2^31)

struct UnionTable {
    const i32 *set_id, *univ;
    const u32 *gs, *ge;
    u32 n;
};

// Two searches of table T side by side (their loads are independent: one loop, two chains in flight): *p = the rows
// whose key (set, gs) lies below ks, known to lie in [*p, hp]; *t = the rows whose key (set, ge) lies below ke, known
// to lie in [*t, ht].  Both keys ascend with the row number; hp, ht <= T.n.
__device__ __forceinline__ void union_rows_below(const UnionTable &T, u64 ks, u64 ke, u32 *p, u32 hp, u32 *t, u32 ht) {
    u32 lp = *p, lt = *t;
    while ((lp < hp) | (lt < ht)) {
        const bool sp = lp < hp, st = lt < ht;
        const u32 mp = sp ? lp + ((hp - lp) >> 1) : 0u, mt = st ? lt + ((ht - lt) >> 1) : 0u;      // (row 0 exists)
        const u64 kp = ((u64)(u32)T.set_id[mp] << 32) | T.gs[mp], kt = ((u64)(u32)T.set_id[mt] << 32) | T.ge[mt];
        if (sp) { if (kp < ks) lp = mp + 1; else hp = mp; }
        if (st) { if (kt < ke) lt = mt + 1; else ht = mt; }
    }
    *p = lp;
    *t = lt;
}

// Blocks 0 .. blocks_a - 1 hold the rows of A (against B), the others the rows of B (against A): which table a lane
// works on is the same in the whole workgroup.  Row r of A has index r in the four arrays, row r of B index A.n + r.
// hflag / tflag: 1 = head / tail (the scans' input; entry A.n + B.n = 0, for the totals); hpos / tpos: the rows of
// the other table below the row's (set, gs) / (set, ge), UN_FLAG set for a head / a tail.
__global__ void __launch_bounds__(256)
union_flag_kernel(UnionTable A, UnionTable B, u32 blocks_a, u32 *__restrict__ hflag, u32 *__restrict__ tflag,
                  u32 *__restrict__ hpos, u32 *__restrict__ tpos) {
    const bool is_a = blockIdx.x < blocks_a;
    const UnionTable X = is_a ? A : B, Y = is_a ? B : A;
    const u32 r = (is_a ? blockIdx.x : blockIdx.x - blocks_a) * blockDim.x + threadIdx.x;
    const u32 at = (is_a ? 0u : A.n) + r;
    const u32 lane = threadIdx.x & 63u;
    const bool valid = r < X.n;
    const ull valid_lanes = __ballot(valid);                 // (a prefix of the wavefront: the rows are consecutive)
    const u32 last = valid_lanes ? 63u - (u32)__clzll(valid_lanes) : 0u;
    i32 sid = 0, un = 0;
    u32 s = 0, e = 0;
    if (valid) { sid = X.set_id[r]; un = X.univ[r]; s = X.gs[r]; e = X.ge[r]; }
    // head: q = the last row of Y that starts before s (A) or at s or before (B) -> p = the rows of Y below that key;
    // tail: q = the first row of Y that ends beyond e (A) or at e or beyond (B) -> t = the rows of Y below that key
    const u64 ks = (((u64)(u32)sid << 32) | s) + (is_a ? 0u : 1u), ke = (((u64)(u32)sid << 32) | e) + (is_a ? 1u : 0u);
    // The keys ascend with the lane, so the positions do: the wavefront's first and last row search the whole table,
    // the rows between them only what lies between those two answers (a few rows where the tables are alike).
    u32 p = 0, t = 0;
    const bool edge = valid && (lane == 0 || lane == last);
    if (edge) union_rows_below(Y, ks, ke, &p, Y.n, &t, Y.n);
    const u32 p0 = (u32)__shfl((int)p, 0, WAVE), p1 = (u32)__shfl((int)p, (int)last, WAVE);
    const u32 t0 = (u32)__shfl((int)t, 0, WAVE), t1 = (u32)__shfl((int)t, (int)last, WAVE);
    if (valid && !edge) {
        p = p0;
        t = t0;
        union_rows_below(Y, ks, ke, &p, p1, &t, t1);
    }
    u32 head = 0, tail = 0;
    if (valid) {
        head = 1;
        if (p > 0 && Y.set_id[p - 1] == sid && Y.univ[p - 1] == un && s <= Y.ge[p - 1]) head = 0;
        tail = 1;
        if (t < Y.n && Y.set_id[t] == sid && Y.univ[t] == un && Y.gs[t] <= e) tail = 0;
        hflag[at] = head;
        tflag[at] = tail;
        hpos[at] = p | (head ? UN_FLAG : 0u);
        tpos[at] = t | (tail ? UN_FLAG : 0u);
    }
    // (no counting here: the scans' last entry is the number of heads / tails, and a counter that every wavefront of
    // two tables adds to is one address for hundreds of thousands of atomics)
    if (blockIdx.x == 0 && threadIdx.x == 0) { hflag[A.n + B.n] = 0; tflag[A.n + B.n] = 0; }
}

// hscan / tscan: the exclusive scans of hflag / tflag (A.n + B.n + 1 entries: A's rows, B's rows, the total).  The
// heads of A before its row r are hscan[r], those of B before its row r hscan[A.n + r] - hscan[A.n]; likewise the tails.
__global__ void __launch_bounds__(256)
union_emit_kernel(UnionTable A, UnionTable B, u32 blocks_a, const u32 *__restrict__ hscan, const u32 *__restrict__ tscan,
                  const u32 *__restrict__ hpos, const u32 *__restrict__ tpos, u32 cap, i32 *__restrict__ o_set,
                  i32 *__restrict__ o_univ, u32 *__restrict__ o_gs, u32 *__restrict__ o_ge) {
    const bool is_a = blockIdx.x < blocks_a;
    const UnionTable X = is_a ? A : B;
    const u32 r = (is_a ? blockIdx.x : blockIdx.x - blocks_a) * blockDim.x + threadIdx.x;
    if (r >= X.n) return;
    const u32 own = is_a ? 0u : A.n, other = is_a ? A.n : 0u;     // first entry of this table, of the other one
    const u32 at = own + r;
    const u32 hp = hpos[at], tp = tpos[at];
    if (hp & UN_FLAG) {
        const u32 o = (hscan[at] - hscan[own]) + (hscan[other + (hp & ~UN_FLAG)] - hscan[other]);
        if (o < cap) { o_set[o] = X.set_id[r]; o_univ[o] = X.univ[r]; o_gs[o] = X.gs[r]; }
    }
    if (tp & UN_FLAG) {
        const u32 o = (tscan[at] - tscan[own]) + (tscan[other + (tp & ~UN_FLAG)] - tscan[other]);
        if (o < cap) o_ge[o] = X.ge[r];
    }
}

// gain0[set] += the lengths of the set's rows (gain0 may be null; sets at and beyond ng have none), info[0] = the
// longest row.  A capped grid strides over the rows, so that the one address of the maximum gets one atomic per
// wavefront of the grid and not one per 64 rows.  The trip count is the same in a whole workgroup and every lane of a
// wavefront stays to the end (the segmented sum needs all 64).
#define UN_SUM_BLOCKS 2048
__global__ void __launch_bounds__(256)
union_sum_kernel(const i32 *__restrict__ set_id, const u32 *__restrict__ gs, const u32 *__restrict__ ge, u32 n,
                 u32 *__restrict__ gain0, u32 ng, ull *__restrict__ info) {
    u32 longest = 0;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < n; base += (u64)gridDim.x * blockDim.x) {
        const u64 r = base + threadIdx.x;
        u32 sid = ~0u, len = 0;
        if (r < n) { sid = (u32)set_id[r]; len = ge[r] - gs[r]; }
        bool last;
        const u32 sum = wave_segsum(len, sid, &last);
        if (gain0 && last && sum && sid < ng) atomicAdd(&gain0[sid], sum);
        longest = max(longest, len);
    }
    longest = wave_max(longest);
    if ((threadIdx.x & 63u) == 0 && longest) atomicMax(&info[0], (ull)longest);
}

extern "C" int catchhip_rows_longest(const catchhip_rows *R, u32 *longest) {
    ARG_CHECK(R && longest);
    if (R->deferred) {
        chip_set_error("rows_longest: deferred rows (a fused scan that was never synchronised)");
        return CATCHHIP_EINVAL;
    }
    *longest = R->lmax;
    return 0;
}

extern "C" int catchhip_rows_union(catchhip_ctx *ctx, const catchhip_rows *Ra, const catchhip_rows *Rb,
                                   catchhip_rows **out, i64 *nrows) {
    ARG_CHECK(ctx && Ra && Rb && out);
    ARG_CHECK(Ra->ctx == ctx && Rb->ctx == ctx);
    *out = nullptr;
    if (nrows) *nrows = 0;
    TRY(chip_rows_form_check(Ra, "rows_union", "the first rows"));
    TRY(chip_rows_form_check(Rb, "rows_union", "the second rows"));
    TRY(chip_space_check(Ra, Rb, "rows_union", "the two tables are not over one coordinate space"));
    TRY(chip_rows_limits_check("rows_union", Ra->total, Ra->n, Rb->n));
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DerivedRows D(ctx, Ra);
    TRY(D.err);
    catchhip_rows *R = D.R.get();
    PhaseTimer &tm = D.tm;
    if (Ra->n == 0 || Rb->n == 0) {                          // the other table, or nothing
        TRY(D.copy_of(Ra->n ? Ra : Rb));
        return D.finish(out, nrows);
    }
    const u32 na = (u32)Ra->n, nb = (u32)Rb->n;
    const size_t nin = (size_t)na + nb;
    const UnionTable A = {Ra->set_id.p, Ra->univ.p, Ra->gs.p, Ra->ge.p, na};
    const UnionTable B = {Rb->set_id.p, Rb->univ.p, Rb->gs.p, Rb->ge.p, nb};
    const u32 blocks_a = (u32)div_up(na, 256), blocks_b = (u32)div_up(nb, 256);
    DevBuf<ull> info;                            // the longest row
    DevBuf<u32> hscan, tscan, hpos, tpos, scan_tmp;
    TRY(info.alloc(1));
    TRY(hscan.alloc(nin + 1));
    TRY(tscan.alloc(nin + 1));
    TRY(hpos.alloc(nin));
    TRY(tpos.alloc(nin));
    HIP_TRY(hipMemsetAsync(info.p, 0, sizeof(ull), s));
    const dim3 grid(blocks_a + blocks_b), blk(256);
    hipLaunchKernelGGL(union_flag_kernel, grid, blk, 0, s, A, B, blocks_a, hscan.p, tscan.p, hpos.p, tpos.p);
    TRY(chip_exclusive_scan_u32(ctx, hscan.p, hscan.p, (i64)nin + 1, scan_tmp));
    TRY(chip_exclusive_scan_u32(ctx, tscan.p, tscan.p, (i64)nin + 1, scan_tmp));
    tm.launch(3);
    HIP_TRY(hipGetLastError());
    // the number of union intervals -- the scans' last entries: heads, tails -- sizes the output: it has to come
    // back before the emit (two words through the pinned staging words, one synchronisation)
    HIP_TRY(hipMemcpyAsync(ctx->h_pin, hscan.p + nin, sizeof(u32), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(ctx->h_pin + 1, tscan.p + nin, sizeof(u32), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const ull ends[2] = {(ull)(u32)ctx->h_pin[0], (ull)(u32)ctx->h_pin[1]};
    if (ends[0] != ends[1]) {
        chip_set_error("rows_union: %llu rows open a union interval and %llu close one; a table is not in the solver's "
                       "form (sorted, its rows disjoint and non-touching inside a set and universe)", ends[0], ends[1]);
        return CATCHHIP_EINVAL;
    }
    if (ends[0] >= (1ull << 31)) {
        chip_set_error("rows_union: the union holds %llu rows; a row table holds fewer than 2^31", ends[0]);
        return CATCHHIP_EINVAL;
    }
    if (ends[0] == 0) {                          // (two non-empty tables in normal form have a first interval)
        chip_set_error("rows_union: no row opens a union interval; a table is not in the solver's form");
        return CATCHHIP_EINVAL;
    }
    const u32 cap = (u32)ends[0];
    const u32 ng = (Ra->gain0_n && Rb->gain0_n) ? std::max(Ra->gain0_n, Rb->gain0_n) : 0u;
    TRY(chip_rows_alloc_soa(R, cap));
    if (ng) {
        TRY(R->gain0.alloc(ng));
        HIP_TRY(hipMemsetAsync(R->gain0.p, 0, sizeof(u32) * (size_t)ng, s));
        R->gain0_n = ng;
    }
    hipLaunchKernelGGL(union_emit_kernel, grid, blk, 0, s, A, B, blocks_a, (const u32 *)hscan.p, (const u32 *)tscan.p,
                       (const u32 *)hpos.p, (const u32 *)tpos.p, cap, R->set_id.p, R->univ.p, R->gs.p, R->ge.p);
    hipLaunchKernelGGL(union_sum_kernel, dim3((unsigned)std::min<i64>(div_up(cap, 256), UN_SUM_BLOCKS)), blk, 0, s, (const i32 *)R->set_id.p,
                       (const u32 *)R->gs.p, (const u32 *)R->ge.p, cap, ng ? R->gain0.p : (u32 *)nullptr, ng, info.p);
    tm.launch(2);
    HIP_TRY(hipGetLastError());
    ull longest = 0;
    tm.stop();
    TRY(chip_read_back(ctx, info.p, sizeof(longest), &longest));
    R->n = (i64)cap;
    R->lmax = (u32)longest;
    return D.finish(out, nrows);
}
