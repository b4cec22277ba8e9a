// What the two pair files of cross.hip's organisation share (cross.hip: the length of a pairing; duplex.hip: its
// nearest-neighbour stability): the packing of records into bit planes, the AND-shift run search, the keys, the
// staging of a call's records and the host side of the four entries.  A file brings its pair kernels and hands their
// launchers over as a CdLaunch; cross.hip's header comment has the organisation.
#pragma once
#include <algorithm>
#include <memory>
#include <vector>

#include "redgraph.h"

#define CD_MAXN (RG_TILE * 16384)      // records of one one-list values call: 16,384 tiles a side

// one 64-character word of a record's three planes
__host__ __device__ static inline void cd_pack_word(const u8 *chars, u32 len, int w, u64 *v, u64 *b0, u64 *b1) {
    u64 xv = 0, x0 = 0, x1 = 0;
    const u32 lo = (u32)w * 64, hi = len < lo + 64 ? len : lo + 64;
    for (u32 i = lo; i < hi; ++i) {
        const u32 c = chars[i];
        xv |= (u64)(c == 'A' || c == 'C' || c == 'G' || c == 'T') << (i - lo);
        x0 |= (u64)((c >> 1) & 1u) << (i - lo);
        x1 |= (u64)((c >> 2) & 1u) << (i - lo);
    }
    *v = xv; *b0 = x0; *b1 = x1;
}

// fwd / rev[(plane * W + w) * npad + record]; word w of a reversed plane is word W - 1 - w of the plain one with its
// bits reversed.  Records beyond n stay zero.
static __global__ void cd_pack_kernel(const u8 *__restrict__ bytes, const i64 *__restrict__ off, u32 n, u32 npad, int W,
                                      u64 *__restrict__ fwd, u64 *__restrict__ rev, u32 *__restrict__ lens) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const i64 a = off[p];
    const u32 len = (u32)(off[p + 1] - a);
    lens[p] = len;
    for (int w = 0; w < W; ++w) {
        u64 v, b0, b1;
        cd_pack_word(bytes + a, len, w, &v, &b0, &b1);
        fwd[((size_t)(0 * W + w)) * npad + p] = v;
        fwd[((size_t)(1 * W + w)) * npad + p] = b0;
        fwd[((size_t)(2 * W + w)) * npad + p] = b1;
        rev[((size_t)(0 * W + (W - 1 - w))) * npad + p] = __brevll(v);
        rev[((size_t)(1 * W + (W - 1 - w))) * npad + p] = __brevll(b0);
        rev[((size_t)(2 * W + (W - 1 - w))) * npad + p] = __brevll(b1);
    }
}

// x &= x >> s over the 64 W bits (0 <= s <= 63; s = 0 leaves x as it is)
template <int W> __host__ __device__ __forceinline__ void cd_and_shift(u64 (&x)[W], u32 s) {
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const u64 hi = w + 1 < W ? x[w + 1] : 0ull;      // (not yet changed: w ascends)
        x[w] &= (x[w] >> s) | ((hi << 1) << (63u - s));
    }
}

// planes.h's RunShifts over 64 W bits: six steps that grow the run in hand 1 -> want <= 64
struct CdSteps {
    u32 want, s0, s1, s2, s3, s4, s5;
    __host__ __device__ __forceinline__ void aim(u32 w) {
        want = w;
        u32 have = 1, s[6];
        for (int k = 0; k < 6; ++k) {                       // (unrolled: s[] stays in registers)
            s[k] = have >= want ? 0u : (have < want - have ? have : want - have);
            have += s[k];
        }
        s0 = s[0]; s1 = s[1]; s2 = s[2]; s3 = s[3]; s4 = s[4]; s5 = s[5];
    }
    // afterwards bit b of x <=> bits b .. b + want - 1 of what x was
    template <int W> __host__ __device__ __forceinline__ void inside(u64 (&x)[W]) const {
        cd_and_shift<W>(x, s0);
        cd_and_shift<W>(x, s1);
        cd_and_shift<W>(x, s2);
        cd_and_shift<W>(x, s3);
        cd_and_shift<W>(x, s4);
        cd_and_shift<W>(x, s5);
    }
};

template <int W> __host__ __device__ __forceinline__ bool cd_any(const u64 (&x)[W]) {
    u64 o = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) o |= x[w];
    return o != 0;
}

// what a pair with `other` as the partner must exceed to change the record that holds `key`
__device__ __forceinline__ int cd_threshold(unsigned long long key, u32 other) {
    const int v = (int)(key >> 32);
    const u32 partner = 0xFFFFFFFFu - (u32)key;
    return v == 0 ? 0 : (other < partner ? v - 1 : v);
}

static __global__ void cd_result_kernel(const unsigned long long *__restrict__ best, u32 n, i32 *__restrict__ value,
                                        i32 *__restrict__ partner) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = best[i];
    const i32 v = (i32)(key >> 32);
    value[i] = v;
    partner[i] = v ? (i32)(0xFFFFFFFFu - (u32)key) : -1;
}

// the records of a call on the device, packed: any bytes, 0 .. RG_MAXLEN characters each
struct CdInput {
    i64 tiles = 0, npad = 0;
    int W = 1;
    DevBuf<u8> d_bytes;
    DevBuf<i64> d_off;
    DevBuf<u64> fwd, rev;
    DevBuf<u32> lens;
};

// What a pair file hands to the entries below: its name in messages, the smallest threshold its graph and flags
// entries take, and the launchers of its two kernels.
//   pairs:   one 64 x 64 tile a block over the upper triangle of one list (values: best; graph: bitmap at `above`)
//   against: a tile of B a block against the range of A's tiles `per` long that blockIdx.y names
struct CdLaunch {
    const char *values_name, *graph_name, *against_name, *flags_name;
    i32 min_above;
    void (*pairs)(hipStream_t s, const CdInput &in, bool graph, i64 n, i32 above, unsigned long long *best,
                  unsigned long long *bitmap);
    void (*against)(hipStream_t s, dim3 grid, bool flags, const CdInput &A, u32 na, u32 per, const CdInput &B, u32 nb,
                    i32 above, unsigned long long *best, u8 *flag);
};

static int cd_check(const char *who, const i64 *off, i64 n, int *W) {
    i64 maxlen = 0;
    for (i64 i = 0; i < n; ++i) {
        const i64 len = off[i + 1] - off[i];
        if (len < 0) { chip_set_error("%s: offsets of record %lld decrease", who, (long long)i); return CATCHHIP_EINVAL; }
        if (len > RG_MAXLEN) {
            chip_set_error("%s: record %lld has %lld characters; the kernel pairs at most %d", who, (long long)i,
                           (long long)len, RG_MAXLEN);
            return CATCHHIP_EINVAL;
        }
        maxlen = std::max(maxlen, len);
    }
    *W = maxlen <= 64 ? 1 : maxlen <= 128 ? 2 : 4;
    return 0;
}

// uploads n >= 1 records on ctx->stream and clears what cd_pack fills; in->W is set
static int cd_stage(catchhip_ctx *ctx, const u8 *bytes, const i64 *off, i64 n, CdInput *in) {
    hipStream_t s = ctx->stream;
    const int W = in->W;
    in->tiles = div_up(n, RG_TILE);
    in->npad = in->tiles * RG_TILE;
    const i64 npad = in->npad, total = off[n] - off[0];
    TRY(in->d_bytes.alloc((size_t)total + 1));
    TRY(in->d_off.alloc((size_t)n + 1));
    TRY(in->fwd.alloc((size_t)3 * W * npad));
    TRY(in->rev.alloc((size_t)3 * W * npad));
    TRY(in->lens.alloc((size_t)npad));
    // (offsets relative to the first byte handed over)
    std::vector<i64> rel((size_t)n + 1);
    for (i64 i = 0; i <= n; ++i) rel[i] = off[i] - off[0];
    if (total) HIP_TRY(hipMemcpyAsync(in->d_bytes.p, bytes + off[0], (size_t)total, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(in->d_off.p, rel.data(), sizeof(i64) * ((size_t)n + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(in->fwd.p, 0, sizeof(u64) * (size_t)3 * W * npad, s));
    HIP_TRY(hipMemsetAsync(in->rev.p, 0, sizeof(u64) * (size_t)3 * W * npad, s));
    HIP_TRY(hipMemsetAsync(in->lens.p, 0, sizeof(u32) * (size_t)npad, s));
    HIP_TRY(hipStreamSynchronize(s));       // (rel[] goes out of scope)
    return 0;
}

static void cd_pack(hipStream_t s, const CdInput &in, i64 n) {
    hipLaunchKernelGGL(cd_pack_kernel, dim3((unsigned)div_up(n, 256)), dim3(256), 0, s, (const u8 *)in.d_bytes.p,
                       (const i64 *)in.d_off.p, (u32)n, (u32)in.npad, in.W, in.fwd.p, in.rev.p, in.lens.p);
}

// the values entry of one list: value / partner of every record (host, n entries each)
static int cd_run_values(catchhip_ctx *ctx, const CdLaunch &L, const u8 *bytes, const i64 *off, i64 n, i32 *value,
                         i32 *partner) {
    if (n > CD_MAXN) {
        chip_set_error("%s: %lld records; one call pairs at most %d (%d tiles a side)", L.values_name, (long long)n, CD_MAXN,
                       CD_MAXN / RG_TILE);
        return CATCHHIP_EINVAL;
    }
    CdInput in;
    TRY(cd_check(L.values_name, off, n, &in.W));
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope pool_scope(ctx);
    hipStream_t s = ctx->stream;
    DevBuf<unsigned long long> best;
    DevBuf<i32> d_out;
    TRY(best.alloc((size_t)div_up(n, RG_TILE) * RG_TILE));
    TRY(d_out.alloc((size_t)2 * n));
    HIP_TRY(hipMemsetAsync(best.p, 0, sizeof(unsigned long long) * (size_t)div_up(n, RG_TILE) * RG_TILE, s));
    TRY(cd_stage(ctx, bytes, off, n, &in));
    PhaseTimer timer(ctx, PHASE_NDF);
    cd_pack(s, in, n);
    L.pairs(s, in, false, n, 0, best.p, nullptr);
    hipLaunchKernelGGL(cd_result_kernel, dim3((unsigned)div_up(n, 256)), dim3(256), 0, s, (const unsigned long long *)best.p,
                       (u32)n, d_out.p, d_out.p + n);
    timer.launch(3);
    timer.stop();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(value, d_out.p, sizeof(i32) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(partner, d_out.p + n, sizeof(i32) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    timer.finish();
    return 0;
}

// the graph entry of one list: the conflict graph of `above` as a catchhip_redgraph
static int cd_run_graph(catchhip_ctx *ctx, const CdLaunch &L, const u8 *bytes, const i64 *off, i64 n, i32 above,
                        catchhip_redgraph **out, i64 *nedges) {
    *out = nullptr;
    if (above < L.min_above) {
        chip_set_error("%s: the threshold must be at least %d (%d)", L.graph_name, L.min_above, above);
        return CATCHHIP_EINVAL;
    }
    CdInput in;
    TRY(cd_check(L.graph_name, off, n, &in.W));
    HIP_TRY(hipSetDevice(ctx->device));
    const i64 tiles = div_up(std::max<i64>(n, 1), RG_TILE);
    const double bitmap_bytes = (double)n * (double)tiles * 8.0;
    if (tiles > 65535 || bitmap_bytes > 0.5 * (double)chip_pool_soft_limit()) {
        chip_set_error("%s: %lld records: the adjacency bitmap (%.1f GB) is larger than half of what the "
                       "device-memory cache may hold (%.1f GB)", L.graph_name, (long long)n, bitmap_bytes / 1e9,
                       (double)chip_pool_soft_limit() / 1e9);
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    hipStream_t s = ctx->stream;
    std::unique_ptr<catchhip_redgraph> G(new catchhip_redgraph());
    G->ctx = ctx;
    G->n = n;
    TRY(G->ptr.alloc((size_t)n + 1));
    if (n == 0) {   // the empty graph
        HIP_TRY(hipMemsetAsync(G->ptr.p, 0, sizeof(i64), s));
        HIP_TRY(hipStreamSynchronize(s));
        TRY(G->idx.alloc(1));
        if (nedges) *nedges = 0;
        *out = G.release();
        return 0;
    }
    DevBuf<u32> deg;
    DevBuf<unsigned long long> bitmap;
    TRY(deg.alloc((size_t)n));
    TRY(bitmap.alloc((size_t)n * tiles));
    HIP_TRY(hipMemsetAsync(bitmap.p, 0, sizeof(unsigned long long) * (size_t)n * tiles, s));
    TRY(cd_stage(ctx, bytes, off, n, &in));
    PhaseTimer timer(ctx, PHASE_NDF);
    cd_pack(s, in, n);
    L.pairs(s, in, true, n, above, nullptr, bitmap.p);
    timer.launch(2);
    TRY(chip_redgraph_from_bitmap(ctx, timer, bitmap.p, tiles, deg.p, G.get()));
    if (nedges) *nedges = G->nedges;
    *out = G.release();
    return 0;
}

#define CA_MAXN ((i64)1 << 30)         // records of either list: the padded count and the tiles stay 32-bit
// Blocks wanted before A's range is split no further: 256 CUs hold 8 blocks of 256 threads each, and blocks end at
// uneven times (the early exits), so the device is level only with several rounds of them -- at 1,563 B tiles and one
// range a CU got 6 or 7 blocks, each as long as the whole stream of A: 1.63 x 10^9 pairs/s for the flags of 100,000
// random 100-mers against 1,000, 2.07 x 10^9 at the 6 ranges this asks for (tools/cross_against_profile.py).
#define CA_FILL 8192

// both two-list entries: checks, both lists packed with one W, the stream of A's tiles; value / partner or flag on
// the host
static int ca_run(catchhip_ctx *ctx, const CdLaunch &L, const u8 *b_bytes, const i64 *b_off, i64 nb, const u8 *a_bytes,
                  const i64 *a_off, i64 na, bool flags, i32 above, i32 *value, i32 *partner, u8 *flag) {
    const char *who = flags ? L.flags_name : L.against_name;
    if (flags && above < L.min_above) {
        chip_set_error("%s: the threshold must be at least %d (%d)", who, L.min_above, above);
        return CATCHHIP_EINVAL;
    }
    if (na > CA_MAXN || nb > CA_MAXN) {
        chip_set_error("%s: %lld records against %lld; one call takes at most %lld in a list", who, (long long)nb,
                       (long long)na, (long long)CA_MAXN);
        return CATCHHIP_EINVAL;
    }
    CdInput A, B;
    TRY(cd_check(who, b_off, nb, &B.W));
    TRY(cd_check(who, a_off, na, &A.W));
    for (i64 i = 0; i < nb; ++i) {                           // an empty A, or nothing to ask
        if (flags) flag[i] = 0;
        else { value[i] = 0; partner[i] = -1; }
    }
    if (na == 0 || nb == 0) return 0;
    A.W = B.W = std::max(A.W, B.W);
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope pool_scope(ctx);
    hipStream_t s = ctx->stream;
    const i64 b_npad = div_up(nb, RG_TILE) * RG_TILE;
    DevBuf<unsigned long long> best;
    DevBuf<i32> d_out;
    DevBuf<u8> d_flag;
    if (flags) {
        TRY(d_flag.alloc((size_t)b_npad));
        HIP_TRY(hipMemsetAsync(d_flag.p, 0, (size_t)b_npad, s));
    } else {
        TRY(best.alloc((size_t)b_npad));
        TRY(d_out.alloc((size_t)2 * nb));
        HIP_TRY(hipMemsetAsync(best.p, 0, sizeof(unsigned long long) * (size_t)b_npad, s));
    }
    TRY(cd_stage(ctx, a_bytes, a_off, na, &A));
    TRY(cd_stage(ctx, b_bytes, b_off, nb, &B));
    // A's tiles in gridDim.y ranges of `per`: one range while B's tiles fill the device by themselves
    const i64 want = std::min<i64>(std::min<i64>(A.tiles, 65535), std::max<i64>(1, div_up((i64)CA_FILL, B.tiles)));
    const u32 per = (u32)div_up(A.tiles, want);
    const dim3 grid((unsigned)B.tiles, (unsigned)div_up(A.tiles, (i64)per));
    PhaseTimer timer(ctx, PHASE_NDF);
    cd_pack(s, A, na);
    cd_pack(s, B, nb);
    L.against(s, grid, flags, A, (u32)na, per, B, (u32)nb, above, best.p, d_flag.p);
    if (!flags)
        hipLaunchKernelGGL(cd_result_kernel, dim3((unsigned)div_up(nb, 256)), dim3(256), 0, s,
                           (const unsigned long long *)best.p, (u32)nb, d_out.p, d_out.p + nb);
    timer.launch(flags ? 3 : 4);
    timer.stop();
    HIP_TRY(hipGetLastError());
    if (flags) {
        HIP_TRY(hipMemcpyAsync(flag, d_flag.p, (size_t)nb, hipMemcpyDeviceToHost, s));
    } else {
        HIP_TRY(hipMemcpyAsync(value, d_out.p, sizeof(i32) * (size_t)nb, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(partner, d_out.p + nb, sizeof(i32) * (size_t)nb, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    timer.finish();
    return 0;
}
