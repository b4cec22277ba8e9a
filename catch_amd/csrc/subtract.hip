// Rows minus the bases another table covers (catchhip_rows_subtract): the reduced set cover instance behind
// SetCoverFilter(fixed_probes=...).
//
// The reference's greedy loop (catch/utils/set_cover.py:362-550) has no notion of sets picked beforehand; picking
// them first is the same as removing their elements from every universe and every other set before the first
// round.  Here that state is a row table: every row [s, t) of `rows` is cut into its maximal runs of bases that no
// row of `covered` touches.  Pieces of one row are at least one covered base apart and stay inside their row, so the
// output keeps the order and the normal form (disjoint, non-touching inside a (set, universe)) of the input and goes
// to catchhip_setcover_greedy as it is.
//
// covered -> bitmap (one bit per base) -> pieces per row (word-parallel) -> exclusive scan -> emit.
// Everything behind the bitmap is chip_rows_cut, which catchhip_rows_below_depth (depth.hip) calls with a bitmap of its
// own and the sets that leave the table whole.
#include <algorithm>

#include "../../include/catchhip_redesign.h"
#include "rows_host.h"
#include "spans.h"
#include "wave.h"

#define SUB_MAXW 5   // rows of at most 5 words (<= 257 bases) load all their words before the first use (RP_MAXW of setcover.hip)

// bit b of bm = base b lies in some row of `covered` (rows of several sets overlap: most words are complete already)
__global__ void __launch_bounds__(256)
sub_bitmap_kernel(const u32 *__restrict__ gs, const u32 *__restrict__ ge, u32 n, unsigned long long *__restrict__ bm) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const u32 s = gs[r], e = ge[r];
    if (e > s) span_paint(bm, s, e);
}

// the uncovered bases of word j of a row's span: v = the bitmap word
__device__ __forceinline__ u64 sub_free(u64 v, const Span &sp, u32 j) { return ~v & span_mask(sp, j); }
// pieces that START in a word: an uncovered base whose predecessor is covered or lies before the row
// (prev = the word before, 0 for the first)
__device__ __forceinline__ u32 sub_starts(u64 f, u64 prev) { return (u32)__popcll(f & ~((f << 1) | (prev >> 63))); }

// skip[s] != 0 (s < nskip; skip may be null): the rows of set s leave the table whole (catchhip_rows_below_depth)
__device__ __forceinline__ bool sub_skipped(const u8 *__restrict__ skip, u32 nskip, i32 sid) {
    return skip && (u32)sid < nskip && skip[(u32)sid];
}

// cnt[r] = pieces of row r; info[0] += their number
__global__ void __launch_bounds__(256)
sub_count_kernel(const i32 *__restrict__ set_id, const u32 *__restrict__ gs, const u32 *__restrict__ ge, u32 n,
                 const unsigned long long *__restrict__ bm, const u8 *__restrict__ skip, u32 nskip,
                 u32 *__restrict__ cnt, unsigned long long *__restrict__ info) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    u32 c = 0;
    if (r < n) {
        const u32 s = gs[r], e = ge[r];
        if (e > s && !sub_skipped(skip, nskip, set_id[r])) {
            const Span sp = span_of(s, e);
            const u32 w0 = sp.w0, nw = sp.nw;
            u64 prev = 0;
            if (nw <= SUB_MAXW) {
                u64 v[SUB_MAXW];
#pragma unroll
                for (u32 j = 0; j < SUB_MAXW; ++j) v[j] = (j < nw) ? bm[w0 + j] : ~0ull;
#pragma unroll
                for (u32 j = 0; j < SUB_MAXW; ++j) {
                    const u64 f = (j < nw) ? sub_free(v[j], sp, j) : 0ull;
                    c += sub_starts(f, prev);
                    prev = f;
                }
            } else {
                for (u32 j = 0; j < nw; ++j) {
                    const u64 f = sub_free(bm[w0 + j], sp, j);
                    c += sub_starts(f, prev);
                    prev = f;
                }
            }
        }
        cnt[r] = c;
    }
    const unsigned long long t = wave_sum((unsigned long long)c);
    if ((threadIdx.x & 63u) == 0 && t) atomicAdd(&info[0], t);
}

// One row's walk over its words, lowest first: word() takes the uncovered bases of a word and the base of its bit 0,
// finish() closes a piece that runs to the row's end.
struct SubWalk {
    i32 *o_set, *o_univ;
    u32 *o_gs, *o_ge;
    u32 o, cap;          // next output row, rows allocated
    i32 sid, un;
    u32 start;           // first base of the open piece
    bool open;
    u32 sum, longest;    // of the pieces written so far
    __device__ __forceinline__ void put(u32 a, u32 b) {
        if (o < cap) { o_set[o] = sid; o_univ[o] = un; o_gs[o] = a; o_ge[o] = b; }
        ++o;
        sum += b - a;
        longest = max(longest, b - a);
    }
    __device__ __forceinline__ void word(u64 f, u32 base) {
        if (open) {
            if (f == ~0ull) return;
            const u32 t = (u32)__builtin_ctzll(~f);
            put(start, base + t);
            open = false;
            f &= ~0ull << t;
        }
        while (f) {
            const u32 b = (u32)__builtin_ctzll(f);
            const u64 x = ~(f >> b);                             // (the b bits shifted in end the run at the word's end)
            const u32 len = x ? (u32)__builtin_ctzll(x) : 64u;
            if (b + len >= 64u) { open = true; start = base + b; return; }
            put(base + b, base + b + len);
            f &= ~0ull << (b + len);
        }
    }
    __device__ __forceinline__ void finish(u32 e) {
        if (open) put(start, e);
        open = false;
    }
};

// the pieces of row r to rows pos[r] .. of the output; their lengths into gain0[set] (the first round's gains of a
// full-coverage solve) and the longest piece into info[1]
__global__ void __launch_bounds__(256)
sub_emit_kernel(const i32 *__restrict__ set_id, const i32 *__restrict__ univ, const u32 *__restrict__ gs,
                const u32 *__restrict__ ge, u32 n, const unsigned long long *__restrict__ bm,
                const u8 *__restrict__ skip, u32 nskip, const u32 *__restrict__ pos, u32 cap, i32 *__restrict__ o_set, i32 *__restrict__ o_univ,
                u32 *__restrict__ o_gs, u32 *__restrict__ o_ge, u32 *__restrict__ gain0, u32 ng,
                unsigned long long *__restrict__ info) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    u32 longest = 0;
    if (r < n) {
        const u32 s = gs[r], e = ge[r];
        SubWalk w;
        w.o_set = o_set; w.o_univ = o_univ; w.o_gs = o_gs; w.o_ge = o_ge;
        w.o = pos[r]; w.cap = cap;
        w.sid = set_id[r]; w.un = univ[r];
        w.start = 0; w.open = false; w.sum = 0; w.longest = 0;
        if (e > s && !sub_skipped(skip, nskip, w.sid)) {
            const Span sp = span_of(s, e);
            const u32 w0 = sp.w0, nw = sp.nw;
            if (nw <= SUB_MAXW) {
                u64 v[SUB_MAXW];
#pragma unroll
                for (u32 j = 0; j < SUB_MAXW; ++j) v[j] = (j < nw) ? bm[w0 + j] : ~0ull;
#pragma unroll
                for (u32 j = 0; j < SUB_MAXW; ++j)
                    if (j < nw) w.word(sub_free(v[j], sp, j), (w0 + j) << 6);
            } else {
                for (u32 j = 0; j < nw; ++j) w.word(sub_free(bm[w0 + j], sp, j), (w0 + j) << 6);
            }
            w.finish(e);
        }
        if (gain0 && w.sum && (u32)w.sid < ng) atomicAdd(&gain0[(u32)w.sid], w.sum);
        longest = w.longest;
    }
    longest = wave_max(longest);
    if ((threadIdx.x & 63u) == 0 && longest) atomicMax(&info[1], (unsigned long long)longest);
}

// a copy of R0 (nothing is covered)
int chip_rows_copy(catchhip_ctx *ctx, const catchhip_rows *R0, catchhip_rows *R) {
    const size_t n = (size_t)R0->n;
    hipStream_t s = ctx->stream;
    TRY(chip_rows_alloc_soa(R, n));
    HIP_TRY(hipMemcpyAsync(R->set_id.p, R0->set_id.p, sizeof(i32) * n, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(R->univ.p, R0->univ.p, sizeof(i32) * n, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(R->gs.p, R0->gs.p, sizeof(u32) * n, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(R->ge.p, R0->ge.p, sizeof(u32) * n, hipMemcpyDeviceToDevice, s));
    if (R0->gain0_n) {
        TRY(R->gain0.alloc(R0->gain0_n));
        HIP_TRY(hipMemcpyAsync(R->gain0.p, R0->gain0.p, sizeof(u32) * (size_t)R0->gain0_n, hipMemcpyDeviceToDevice, s));
        R->gain0_n = R0->gain0_n;
    }
    HIP_TRY(hipStreamSynchronize(s));
    R->n = R0->n;
    R->lmax = R0->lmax;
    return 0;
}

// The rows of R0 (a non-empty table that passed chip_rows_form_check, fewer than 2^31 rows) cut into their maximal
// runs of bases whose bit in bm is clear, into R (made by chip_rows_new over R0's coordinate space); the rows of the
// sets with skip[set] != 0 (set < nskip; skip may be null) are left out whole.  count -> exclusive scan -> read-back
// of the number of pieces -> emit; R gets n, lmax and, when R0 has it, gain0.  tm is the caller's running timer: its
// stop event is recorded behind the emit.
int chip_rows_cut(catchhip_ctx *ctx, const catchhip_rows *R0, const unsigned long long *bm, const u8 *skip, u32 nskip,
                  catchhip_rows *R, PhaseTimer &tm, const char *who) {
    hipStream_t s = ctx->stream;
    const u32 n0 = (u32)R0->n;
    DevBuf<unsigned long long> info;
    DevBuf<u32> cnt, pos, scan_tmp;
    TRY(info.alloc(2));
    TRY(cnt.alloc(n0));
    TRY(pos.alloc(n0));
    HIP_TRY(hipMemsetAsync(info.p, 0, sizeof(unsigned long long) * 2, s));
    const dim3 grid((unsigned)div_up(n0, 256)), blk(256);
    hipLaunchKernelGGL(sub_count_kernel, grid, blk, 0, s, (const i32 *)R0->set_id.p, (const u32 *)R0->gs.p,
                       (const u32 *)R0->ge.p, n0, bm, skip, nskip, cnt.p, info.p);
    TRY(chip_exclusive_scan_u32(ctx, cnt.p, pos.p, n0, scan_tmp));
    tm.launch(2);
    HIP_TRY(hipGetLastError());
    // the number of pieces sizes the output (a row may fall into many): it has to come back before the emit
    unsigned long long npieces = 0;
    TRY(chip_read_back(ctx, info.p, sizeof(npieces), &npieces));
    if (npieces >= (1ull << 31)) {
        chip_set_error("%s: the rows fall into %llu pieces; a row table holds fewer than 2^31", who, npieces);
        return CATCHHIP_EINVAL;
    }
    if (npieces) {
        const u32 cap = (u32)npieces, ng = R0->gain0_n;
        TRY(chip_rows_alloc_soa(R, cap));
        if (ng) {
            TRY(R->gain0.alloc(ng));
            HIP_TRY(hipMemsetAsync(R->gain0.p, 0, sizeof(u32) * (size_t)ng, s));
            R->gain0_n = ng;
        }
        hipLaunchKernelGGL(sub_emit_kernel, grid, blk, 0, s, (const i32 *)R0->set_id.p, (const i32 *)R0->univ.p,
                           (const u32 *)R0->gs.p, (const u32 *)R0->ge.p, n0, bm, skip, nskip, (const u32 *)pos.p, cap,
                           R->set_id.p, R->univ.p, R->gs.p, R->ge.p, ng ? R->gain0.p : (u32 *)nullptr, ng, info.p);
        tm.launch(1);
        HIP_TRY(hipGetLastError());
        unsigned long long longest = 0;
        tm.stop();
        TRY(chip_read_back(ctx, info.p + 1, sizeof(longest), &longest));
        R->n = (i64)cap;
        R->lmax = (u32)longest;
    }
    return 0;
}

// ---- rows without some sets (catchhip_rows_drop_sets; include/catchhip_redesign.h) -----------------------------------
// No row is cut: a row stays or goes with its set, so count / scan / emit move whole rows and need no bitmap.
// cnt[r] = 1 iff row r stays; info[0] += the rows that stay, info[2] = 1 if a row's set id is not below num_sets
__global__ void __launch_bounds__(256)
drop_count_kernel(const i32 *__restrict__ set_id, const u32 *__restrict__ gs, const u32 *__restrict__ ge, u32 n,
                  const u8 *__restrict__ drop, u32 num_sets, u32 *__restrict__ cnt, unsigned long long *__restrict__ info) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    u32 c = 0;
    if (r < n) {
        const u32 sid = (u32)set_id[r];
        if (sid >= num_sets) info[2] = 1ull;                 // (every writer writes 1)
        else c = (ge[r] > gs[r] && !drop[sid]) ? 1u : 0u;
        cnt[r] = c;
    }
    const unsigned long long t = wave_sum((unsigned long long)c);
    if ((threadIdx.x & 63u) == 0 && t) atomicAdd(&info[0], t);
}

// row r to row pos[r] of the output where cnt[r]; lengths into gain0[set], the longest into info[1]
__global__ void __launch_bounds__(256)
drop_emit_kernel(const i32 *__restrict__ set_id, const i32 *__restrict__ univ, const u32 *__restrict__ gs,
                 const u32 *__restrict__ ge, u32 n, const u32 *__restrict__ cnt, const u32 *__restrict__ pos, u32 cap,
                 i32 *__restrict__ o_set, i32 *__restrict__ o_univ, u32 *__restrict__ o_gs, u32 *__restrict__ o_ge,
                 u32 *__restrict__ gain0, u32 ng, unsigned long long *__restrict__ info) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    u32 longest = 0;
    if (r < n && cnt[r]) {
        const u32 o = pos[r], s = gs[r], e = ge[r];
        const i32 sid = set_id[r];
        if (o < cap) { o_set[o] = sid; o_univ[o] = univ[r]; o_gs[o] = s; o_ge[o] = e; }
        if (gain0 && (u32)sid < ng) atomicAdd(&gain0[(u32)sid], e - s);
        longest = e - s;
    }
    longest = wave_max(longest);
    if ((threadIdx.x & 63u) == 0 && longest) atomicMax(&info[1], (unsigned long long)longest);
}

extern "C" int catchhip_rows_drop_sets(catchhip_ctx *ctx, const catchhip_rows *R0, i64 num_sets, const u8 *drop,
                                       catchhip_rows **out, i64 *nrows) {
    ARG_CHECK(ctx && R0 && out);
    ARG_CHECK(R0->ctx == ctx);
    *out = nullptr;
    if (nrows) *nrows = 0;
    ARG_CHECK(num_sets >= 0 && num_sets < ((i64)1 << 31) && (num_sets == 0 || drop));
    TRY(chip_rows_form_check(R0, "rows_drop_sets", "the rows"));
    TRY(chip_rows_limits_check("rows_drop_sets", R0->total, R0->n));
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DerivedRows D(ctx, R0);
    TRY(D.err);
    catchhip_rows *R = D.R.get();
    if (R0->n == 0) {                                        // nothing to drop from
        TRY(D.copy_of(R0));
        return D.finish(out, nrows);
    }
    const u32 n0 = (u32)R0->n;
    DevBuf<u8> d_drop;
    DevBuf<unsigned long long> info;
    DevBuf<u32> cnt, pos, scan_tmp;
    TRY(d_drop.alloc((size_t)num_sets + 1));
    TRY(info.alloc(3));
    TRY(cnt.alloc(n0));
    TRY(pos.alloc(n0));
    if (num_sets) HIP_TRY(hipMemcpyAsync(d_drop.p, drop, (size_t)num_sets, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(info.p, 0, sizeof(unsigned long long) * 3, s));
    const dim3 grid((unsigned)div_up(n0, 256)), blk(256);
    hipLaunchKernelGGL(drop_count_kernel, grid, blk, 0, s, (const i32 *)R0->set_id.p, (const u32 *)R0->gs.p,
                       (const u32 *)R0->ge.p, n0, (const u8 *)d_drop.p, (u32)num_sets, cnt.p, info.p);
    TRY(chip_exclusive_scan_u32(ctx, cnt.p, pos.p, n0, scan_tmp));
    D.tm.launch(2);
    HIP_TRY(hipGetLastError());
    unsigned long long head[3] = {0, 0, 0};                  // (also: `drop` is the caller's again)
    TRY(chip_read_back(ctx, info.p, sizeof(head), head));
    if (head[2]) {
        chip_set_error("rows_drop_sets: a row's set id is not below the %lld flags given", (long long)num_sets);
        return CATCHHIP_EINVAL;
    }
    const u32 cap = (u32)head[0], ng = R0->gain0_n;
    if (ng) {                                                // carried whatever stays
        TRY(R->gain0.alloc(ng));
        HIP_TRY(hipMemsetAsync(R->gain0.p, 0, sizeof(u32) * (size_t)ng, s));
        R->gain0_n = ng;
    }
    if (cap) {
        TRY(chip_rows_alloc_soa(R, cap));
        hipLaunchKernelGGL(drop_emit_kernel, grid, blk, 0, s, (const i32 *)R0->set_id.p, (const i32 *)R0->univ.p,
                           (const u32 *)R0->gs.p, (const u32 *)R0->ge.p, n0, (const u32 *)cnt.p, (const u32 *)pos.p, cap,
                           R->set_id.p, R->univ.p, R->gs.p, R->ge.p, ng ? R->gain0.p : (u32 *)nullptr, ng, info.p);
        D.tm.launch(1);
        HIP_TRY(hipGetLastError());
        unsigned long long longest = 0;
        D.tm.stop();
        TRY(chip_read_back(ctx, info.p + 1, sizeof(longest), &longest));
        R->n = (i64)cap;
        R->lmax = (u32)longest;
    } else {
        D.tm.stop();
        HIP_TRY(hipStreamSynchronize(s));
    }
    return D.finish(out, nrows);
}

extern "C" int catchhip_rows_subtract(catchhip_ctx *ctx, const catchhip_rows *R0, const catchhip_rows *C,
                                      catchhip_rows **out, i64 *nrows) {
    ARG_CHECK(ctx && R0 && C && out);
    ARG_CHECK(R0->ctx == ctx && C->ctx == ctx);
    *out = nullptr;
    if (nrows) *nrows = 0;
    TRY(chip_rows_form_check(R0, "rows_subtract", "the rows"));
    TRY(chip_rows_form_check(C, "rows_subtract", "the covered rows"));
    TRY(chip_space_check(C, R0, "rows_subtract", "the covered rows are not over the coordinate space of the rows"));
    TRY(chip_rows_limits_check("rows_subtract", R0->total, R0->n, C->n));
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    DerivedRows D(ctx, R0);
    TRY(D.err);
    if (R0->n == 0 || C->n == 0) {                           // nothing to cut, or nothing covered: a copy
        TRY(D.copy_of(R0));
        return D.finish(out, nrows);
    }
    const u32 nc = (u32)C->n;
    DevBuf<unsigned long long> bm;
    TRY(chip_cut_bitmap(ctx, R0->total, true, bm));
    hipLaunchKernelGGL(sub_bitmap_kernel, dim3((unsigned)div_up(nc, 256)), dim3(256), 0, ctx->stream, (const u32 *)C->gs.p,
                       (const u32 *)C->ge.p, nc, bm.p);
    D.tm.launch(1);
    TRY(chip_rows_cut(ctx, R0, (const unsigned long long *)bm.p, nullptr, 0, D.R.get(), D.tm, "rows_subtract"));
    return D.finish(out, nrows);
}
