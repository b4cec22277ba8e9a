// The wanted bases of a coordinate space (catchhip_basemask_*) and the rows cut to them (catchhip_rows_restrict): the
// device side of SetCoverFilter(target_regions=...).
//
// The other two cuts of a row table (subtract.hip, depth.hip) get "these bases need no cover" from ROWS: a lane per row
// ORs the row's words into a zeroed bitmap, which is right for rows of at most 257 bases.  Here it comes from
// INTERVALS of any length (a gene, a chromosome without its repeats), so the bitmap is built the other way round:
//
//   bm_build_kernel   a lane per 64-bit word of the bitmap, consecutive lanes on consecutive words.  The lane finds
//                     the first interval that ends beyond its word's first base (a binary search over the sorted ends)
//                     and ORs in the intervals that start before the word's end -- at most 32 of them, since intervals
//                     do not touch.  Every word is computed in registers and stored once: no memset, no atomics on
//                     the bitmap, and no loop whose trip count grows with an interval's length.  The words behind the
//                     last base (the padding chip_rows_cut may read) are stored as all ones by the same launch.
//                     The wanted bases per universe are counted from the finished words before they leave the
//                     registers: a wavefront (64 words = 4,096 bases) that lies in one universe reduces its
//                     popcounts and issues one atomicAdd; one that holds universe boundaries (they are not
//                     word-aligned) walks the universes it touches, one reduction and one atomicAdd per universe.
//   chip_rows_cut     subtract.hip's count, scan and emit over that bitmap (catchhip_rows_restrict)
//
// Integer arithmetic only, and the atomics commute: the result does not depend on the launch geometry.  Scratch beyond
// the bitmap: the interval boundaries (8 bytes per interval) and 12 bytes per universe.
#include <algorithm>

#include "rows_host.h"
#include "spans.h"
#include "wave.h"

typedef unsigned long long ull;

// gs / ge: the n intervals in global coordinates, ascending, each start greater than the end before it; bm: nwords
// words; wanted[ng]: zeroed by the caller.  Every lane of a wavefront stays to the end (the reductions need all 64).
__global__ void __launch_bounds__(256)
bm_build_kernel(const u32 *__restrict__ gs, const u32 *__restrict__ ge, u32 n, u64 total, u32 nwords,
                const u32 *__restrict__ genome_off, u32 ng, ull *__restrict__ bm, ull *__restrict__ wanted) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 lane = threadIdx.x & 63u;
    const u64 base = (u64)w << 6;
    u64 want = 0;
    if (w < nwords && base < total) {
        u32 lo = 0, hi = n;                                  // the first interval with ge > base
        while (lo < hi) {
            const u32 mid = lo + ((hi - lo) >> 1);
            if ((u64)ge[mid] > base) hi = mid; else lo = mid + 1;
        }
        for (u32 i = lo; i < n; ++i) {
            const u64 a = gs[i];
            if (a >= base + 64) break;
            want |= span_in_word(base, a, (u64)ge[i]);
        }
    }
    if (w < nwords) bm[w] = ~want;
    // the wanted bases per universe, from the words this wavefront holds
    const u64 wbase = (u64)(w - lane) << 6, wend = wbase + 64ull * WAVE;
    if (wbase >= total || ng == 0) return;                   // (the whole wavefront)
    u32 u0 = 0;
    if (lane == 0) u0 = find_segment(genome_off, ng, (u32)wbase);
    u0 = (u32)__shfl((int)u0, 0, WAVE);
    if ((u64)genome_off[u0 + 1] >= min(wend, total)) {       // one universe
        const ull t = wave_sum((ull)__popcll(want));
        if (lane == 0 && t) atomicAdd(&wanted[u0], t);
        return;
    }
    for (u32 u = u0; u < ng; ++u) {
        const u64 a = genome_off[u], b = genome_off[u + 1];
        if (a >= wend) break;
        u64 m = 0;
        if (b > a && a < base + 64 && b > base) m = span_in_word(base, a, b);
        const ull t = wave_sum((ull)__popcll(want & m));
        if (lane == 0 && t) atomicAdd(&wanted[u], t);
    }
}

extern "C" int catchhip_basemask_create(catchhip_ctx *ctx, const i64 *genome_len, i32 ngenomes, const i32 *universe,
                                        const i64 *start, const i64 *end, i64 n, catchhip_basemask **out,
                                        i64 *wanted_per_universe) {
    ARG_CHECK(ctx && out && n >= 0 && ngenomes >= 0 && (ngenomes == 0 || genome_len));
    ARG_CHECK(n == 0 || (universe && start && end));
    *out = nullptr;
    std::unique_ptr<catchhip_basemask> M(new catchhip_basemask());
    M->ctx = ctx;
    M->ngenomes = ngenomes;
    M->h_genome_off.assign((size_t)ngenomes + 1, 0);
    for (i32 g = 0; g < ngenomes; ++g) {
        if (genome_len[g] < 0) { chip_set_error("basemask_create: negative universe length"); return CATCHHIP_EINVAL; }
        M->h_genome_off[g + 1] = M->h_genome_off[g] + genome_len[g];
    }
    M->total = M->h_genome_off[ngenomes];
    if (M->total >= ((i64)1 << 32) - 1) {
        chip_set_error("basemask_create: more than 2^32 - 2 target bases");
        return CATCHHIP_EINVAL;
    }
    if (n >= ((i64)1 << 31)) { chip_set_error("basemask_create: too many intervals"); return CATCHHIP_EINVAL; }
    std::vector<u32> gs((size_t)n), ge((size_t)n), go((size_t)ngenomes + 1);
    for (i32 g = 0; g <= ngenomes; ++g) go[g] = (u32)M->h_genome_off[g];
    for (i64 i = 0; i < n; ++i) {
        const i32 u = universe[i];
        const char *what = nullptr;
        if (u < 0 || u >= ngenomes) what = "names a universe out of range";
        else if (start[i] < 0 || end[i] <= start[i]) what = "is empty or negative";
        else if (end[i] > genome_len[u]) what = "ends beyond its universe";
        else if (i > 0 && u < universe[i - 1]) what = "is out of order";
        else if (i > 0 && u == universe[i - 1] && start[i] <= end[i - 1])
            what = start[i] < start[i - 1] ? "is out of order" : "overlaps or touches the one before it";
        if (what) {
            chip_set_error("basemask_create: interval %lld (universe %d, [%lld, %lld)) %s", (long long)i, (int)u,
                           (long long)start[i], (long long)end[i], what);
            return CATCHHIP_EINVAL;
        }
        gs[i] = (u32)(M->h_genome_off[u] + start[i]);
        ge[i] = (u32)(M->h_genome_off[u] + end[i]);
    }
    if (wanted_per_universe) for (i32 u = 0; u < ngenomes; ++u) wanted_per_universe[u] = 0;
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t nwords = chip_cut_bitmap_words(M->total);
    const size_t ngu = (size_t)ngenomes;
    DevBuf<u32> d_gs, d_ge, d_go;
    DevBuf<ull> d_wanted;
    TRY(chip_cut_bitmap(ctx, M->total, false, M->unwanted));  // (the kernel stores every word)
    TRY(d_gs.alloc((size_t)n));
    TRY(d_ge.alloc((size_t)n));
    TRY(d_go.alloc(ngu + 1));
    TRY(d_wanted.alloc(ngu));
    PhaseTimer tm(ctx, PHASE_ROWS);
    if (n) {
        HIP_TRY(hipMemcpyAsync(d_gs.p, gs.data(), sizeof(u32) * (size_t)n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_ge.p, ge.data(), sizeof(u32) * (size_t)n, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(d_go.p, go.data(), sizeof(u32) * (ngu + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_wanted.p, 0, sizeof(ull) * (ngu ? ngu : 1), s));
    hipLaunchKernelGGL(bm_build_kernel, dim3((unsigned)div_up((i64)nwords, 256)), dim3(256), 0, s, (const u32 *)d_gs.p,
                       (const u32 *)d_ge.p, (u32)n, (u64)M->total, (u32)nwords, (const u32 *)d_go.p, (u32)ngenomes,
                       M->unwanted.p, d_wanted.p);
    tm.launch(1);
    HIP_TRY(hipGetLastError());
    tm.stop();
    TRY(chip_fetch_counters(ctx, d_wanted.p, ngu, wanted_per_universe));    // (also: the pageable gs / ge / go have been read)
    tm.finish();
    *out = M.release();
    return 0;
}

extern "C" int catchhip_basemask_fetch(catchhip_ctx *ctx, const catchhip_basemask *mask, uint64_t *words) {
    ARG_CHECK(ctx && mask && mask->ctx == ctx);
    const size_t nw = (size_t)((mask->total + 63) / 64);
    if (nw == 0) return 0;
    ARG_CHECK(words);
    HIP_TRY(hipSetDevice(ctx->device));
    TRY(chip_pinned_reserve(ctx, sizeof(ull) * nw));
    HIP_TRY(hipMemcpyAsync(ctx->h_big, mask->unwanted.p, sizeof(ull) * nw, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(words, ctx->h_big, sizeof(ull) * nw);
    return 0;
}

extern "C" int catchhip_basemask_destroy(catchhip_basemask *mask) {
    if (mask) { (void)hipSetDevice(mask->ctx->device); delete mask; }
    return 0;
}

extern "C" int catchhip_rows_restrict(catchhip_ctx *ctx, const catchhip_rows *R0, const catchhip_basemask *mask,
                                      catchhip_rows **out, i64 *nrows) {
    ARG_CHECK(ctx && R0 && mask && out);
    ARG_CHECK(R0->ctx == ctx && mask->ctx == ctx);
    *out = nullptr;
    if (nrows) *nrows = 0;
    TRY(chip_rows_form_check(R0, "rows_restrict", "the rows"));
    TRY(chip_space_check(mask, R0, "rows_restrict", "the mask is not over the coordinate space of the rows"));
    TRY(chip_rows_limits_check("rows_restrict", R0->total, R0->n));
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    DerivedRows D(ctx, R0);
    TRY(D.err);
    if (R0->n) TRY(chip_rows_cut(ctx, R0, (const ull *)mask->unwanted.p, nullptr, 0, D.R.get(), D.tm, "rows_restrict"));
    else TRY(D.copy_of(nullptr));
    return D.finish(out, nrows);
}
