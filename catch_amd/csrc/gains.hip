// Gain per pick (catchhip_rows_pick_gains): how many bases each pick of a pick list covered for the first time when
// it was taken, and the coverage reached after the first k picks, behind SetCoverFilter(pick_gains=True / max_probes=N)
// and `design --max-probes / --write-coverage-curve`.
//
// rank(i) = i, the position in the pick list.  first(b) = the smallest rank among the picks whose set has a row over
// base b.  gains[i] = the bases b with first(b) == i.  For a checkpoint k and a universe u, cov_u(k) = covered0[u] +
// the bases of u with first(b) < k; per checkpoint the sum over the universes and the universe with the smallest
// cov_u / denom[u] are reported.
//
//   1. chip_depth_marks (depth.hip)  the pick table: rank[set] = position of the pick of that set (GN_NONE: not
//                                    picked); a pick out of range or given twice is refused
//   2. gn_first_kernel               first[] = u32 per base, all ones beforehand.  A wavefront per row of a picked
//                                    set, its lanes on consecutive bases: every wave instruction reads and (where the
//                                    row's rank is lower) atomicMin's a contiguous 256 bytes
//   3. gn_count_kernel               again a wavefront per picked row: __ballot(first[b] == rank) and its popcount
//                                    summed over the row, then ONE atomicAdd into gains[rank] and, with checkpoints,
//                                    one into table[j][universe], j = the first checkpoint above the rank
//                                    (find_segment).  The rows of one set do not overlap: each base counts once.
//   4. gn_prefix_kernel              a lane per universe, running sum over j from covered0[u]: table[j][u] = cov_u(k_j)
//                                    (the table lies [j][u]: the lanes of a wavefront read neighbouring words)
//   5. gn_reduce_kernel              a workgroup per checkpoint: the sum over the universes and the argmin of
//                                    cov_u / denom[u] by exact 64-bit cross-multiplication, ties to the lower universe
//
// Everything is integer arithmetic; atomicMin and atomicAdd on integers commute, so the result depends neither on
// the launch geometry nor on the order of the atomics.  Scratch: 4 bytes per target base (first[]) plus 4 bytes x
// checkpoints x universes (the table).  Tables of up to 2^31 - 1 rows: the two row passes compute the row of a
// wavefront in 64 bits.
#include "rows_host.h"
#include "wave.h"

#define GN_NONE CHIP_NOT_PICKED

// One row's bases by one wavefront: *rk = the rank of its set (GN_NONE: not picked, or a set id out of range),
// [*a, *b) = its bases, cut at `total`
__device__ __forceinline__ void gn_row(const i32 *__restrict__ set_id, const u32 *__restrict__ gs,
                                       const u32 *__restrict__ ge, u32 r, u32 num_sets, const u32 *__restrict__ rank,
                                       u32 total, u32 *rk, u32 *a, u32 *b) {
    const u32 s = (u32)set_id[r];
    *rk = s < num_sets ? rank[s] : GN_NONE;
    *a = gs[r];
    *b = min(ge[r], total);
}

__global__ void __launch_bounds__(256)
gn_first_kernel(const i32 *__restrict__ set_id, const u32 *__restrict__ gs, const u32 *__restrict__ ge, u32 n,
                u32 num_sets, const u32 *__restrict__ rank, u32 total, u32 *__restrict__ first) {
    // (64-bit: the grid has n / 4 workgroups, and blockIdx.x * 256 passes 2^32 from 2^26 rows on)
    const i64 r64 = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r64 >= (i64)n) return;                               // (the whole wavefront)
    const u32 r = (u32)r64, lane = threadIdx.x & 63u;
    u32 rk, a, b;
    gn_row(set_id, gs, ge, r, num_sets, rank, total, &rk, &a, &b);
    if (rk == GN_NONE || b <= a) return;
    const u32 len = b - a;
    for (u32 o = lane; o < len; o += WAVE) {                 // (offsets: a + o stays below total)
        if (first[a + o] > rk) atomicMin(&first[a + o], rk);
    }
}

// ck_off = {0, k_0, ..., k_{ncheck-1}} (ncheck + 1 entries; null: no checkpoints); table[j * ng + u]
__global__ void __launch_bounds__(256)
gn_count_kernel(const i32 *__restrict__ set_id, const i32 *__restrict__ univ, const u32 *__restrict__ gs,
                const u32 *__restrict__ ge, u32 n, u32 num_sets, const u32 *__restrict__ rank, u32 total,
                const u32 *__restrict__ first, u32 *__restrict__ gains, const u32 *__restrict__ ck_off, u32 ncheck,
                u32 ng, u32 *__restrict__ table) {
    // (64-bit: the grid has n / 4 workgroups, and blockIdx.x * 256 passes 2^32 from 2^26 rows on)
    const i64 r64 = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r64 >= (i64)n) return;                               // (the whole wavefront)
    const u32 r = (u32)r64, lane = threadIdx.x & 63u;
    u32 rk, a, b;
    gn_row(set_id, gs, ge, r, num_sets, rank, total, &rk, &a, &b);
    if (rk == GN_NONE || b <= a) return;
    const u32 len = b - a;
    u32 cnt = 0;
    for (u32 o0 = 0; o0 < len; o0 += WAVE) {                 // (uniform trip count: the ballot sees every lane)
        const u32 o = o0 + lane;
        cnt += (u32)__popcll(__ballot(o < len && first[a + o] == rk));
    }
    if (lane != 0 || cnt == 0) return;
    atomicAdd(&gains[rk], cnt);
    if (ncheck && rk < ck_off[ncheck]) {                     // (a rank at or past the last checkpoint counts nowhere)
        const u32 u = (u32)univ[r];
        if (u < ng) atomicAdd(&table[(size_t)find_segment(ck_off, ncheck, rk) * ng + u], cnt);
    }
}

// table[j][u]: the bases of u first covered by the ranks in [k_{j-1}, k_j)  ->  cov_u(k_j)
__global__ void __launch_bounds__(256)
gn_prefix_kernel(u32 *__restrict__ table, u32 ncheck, u32 ng, const u32 *__restrict__ covered0) {
    const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= ng) return;
    u32 run = covered0 ? covered0[u] : 0u;
    for (u32 j = 0; j < ncheck; ++j) {
        run += table[(size_t)j * ng + u];
        table[(size_t)j * ng + u] = run;
    }
}

// is (ca / da, universe ua) worse covered than (cb / db, ub)?  da, db > 0; GN_NONE as a universe: nobody yet
__device__ __forceinline__ bool gn_worse(u32 ca, u32 da, u32 ua, u32 cb, u32 db, u32 ub) {
    if (ua == GN_NONE) return false;
    if (ub == GN_NONE) return true;
    const u64 l = (u64)ca * db, r = (u64)cb * da;            // ca / da < cb / db  <=>  ca * db < cb * da
    return l < r || (l == r && ua < ub);
}

// out[3 * j] = sum over u of cov_u(k_j), out[3 * j + 1] = the worst universe (GN_NONE widened: none), out[3 * j + 2] =
// its cov.  A workgroup per checkpoint.
__global__ void __launch_bounds__(256)
gn_reduce_kernel(const u32 *__restrict__ table, u32 ng, const u32 *__restrict__ denom, u64 *__restrict__ out) {
    __shared__ u64 s_sum[256 / WAVE];
    __shared__ u32 s_c[256 / WAVE], s_d[256 / WAVE], s_u[256 / WAVE];
    const u32 j = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u32 *row = table + (size_t)j * ng;
    u64 sum = 0;
    u32 bc = 0, bd = 1, bu = GN_NONE;
    for (u32 u = tid; u < ng; u += 256) {                    // (ascending u per thread: a tie keeps the lower one)
        const u32 c = row[u], d = denom[u];
        sum += c;
        if (d && gn_worse(c, d, u, bc, bd, bu)) { bc = c; bd = d; bu = u; }
    }
    sum = wave_sum(sum);
    for (int d = 32; d > 0; d >>= 1) {
        const u32 oc = __shfl_down(bc, d, WAVE), od = __shfl_down(bd, d, WAVE), ou = __shfl_down(bu, d, WAVE);
        if (gn_worse(oc, od, ou, bc, bd, bu)) { bc = oc; bd = od; bu = ou; }
    }
    if (lane == 0) { s_sum[wave] = sum; s_c[wave] = bc; s_d[wave] = bd; s_u[wave] = bu; }
    __syncthreads();
    if (tid != 0) return;
    for (u32 w = 1; w < 256 / WAVE; ++w) {
        sum += s_sum[w];
        if (gn_worse(s_c[w], s_d[w], s_u[w], bc, bd, bu)) { bc = s_c[w]; bd = s_d[w]; bu = s_u[w]; }
    }
    out[3 * (size_t)j] = sum;
    out[3 * (size_t)j + 1] = bu;
    out[3 * (size_t)j + 2] = bu == GN_NONE ? 0u : bc;
}

extern "C" int catchhip_rows_pick_gains(catchhip_ctx *ctx, const catchhip_rows *R0, i64 num_sets, const i64 *picks,
                                        i64 npicks, u32 *gains, const i64 *checkpoints, i64 ncheck, const i64 *denom,
                                        const i64 *covered0, u64 *covered_total, i32 *worst_universe,
                                        i64 *worst_covered) {
    ARG_CHECK(ctx && R0);
    ARG_CHECK(R0->ctx == ctx);
    ARG_CHECK(num_sets >= 0 && num_sets < ((i64)1 << 31) && npicks >= 0 && ncheck >= 0);
    ARG_CHECK(npicks == 0 || (picks && gains));
    ARG_CHECK(ncheck == 0 || (checkpoints && denom && covered_total && worst_universe && worst_covered));
    TRY(chip_depth_check(R0, num_sets, npicks, 1, "rows_pick_gains"));
    const i64 ng = R0->ngenomes;
    if (ncheck && npicks == 0) {
        chip_set_error("rows_pick_gains: %lld checkpoints of an empty pick list", (long long)ncheck);
        return CATCHHIP_EINVAL;
    }
    for (i64 j = 0; j < ncheck; ++j) {
        if (checkpoints[j] < 1 || checkpoints[j] > npicks) {
            chip_set_error("rows_pick_gains: checkpoint %lld lies outside 1 .. %lld picks", (long long)checkpoints[j],
                           (long long)npicks);
            return CATCHHIP_EINVAL;
        }
        if (j && checkpoints[j] <= checkpoints[j - 1]) {
            chip_set_error("rows_pick_gains: the checkpoints are not strictly ascending (%lld after %lld)",
                           (long long)checkpoints[j], (long long)checkpoints[j - 1]);
            return CATCHHIP_EINVAL;
        }
    }
    if (ncheck && ncheck * (ng > 0 ? ng : 1) >= ((i64)1 << 31)) {
        chip_set_error("rows_pick_gains: %lld checkpoints x %lld universes is 2^31 table entries or more; "
                       "split the checkpoints", (long long)ncheck, (long long)ng);
        return CATCHHIP_EINVAL;
    }
    if (ncheck) {
        // cov_u and denom[u] are the two factors of the exact comparison: both below 2^32
        for (i64 u = 0; u < ng; ++u) {
            const i64 len = R0->h_genome_off[(size_t)u + 1] - R0->h_genome_off[(size_t)u];
            const i64 c0 = covered0 ? covered0[u] : 0;
            if (denom[u] < 0 || denom[u] >= ((i64)1 << 32) || c0 < 0 || c0 + len >= ((i64)1 << 32)) {
                chip_set_error("rows_pick_gains: universe %lld: denom %lld / covered0 %lld do not fit 32 bits",
                               (long long)u, (long long)denom[u], (long long)c0);
                return CATCHHIP_EINVAL;
            }
        }
    }
    if (npicks == 0) return 0;
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    PhaseTimer tm(ctx, PHASE_ROWS);
    const u32 np = (u32)npicks, ns = (u32)num_sets, n0 = (u32)R0->n, nc = (u32)ncheck, ngu = (u32)ng;
    const u32 total = (u32)R0->total;
    DevBuf<i64> d_picks;
    DevBuf<u32> rank;
    DevBuf<u8> picked;
    TRY(chip_depth_marks(ctx, picks, npicks, num_sets, d_picks, rank, picked, tm, "rows_pick_gains"));
    DevBuf<u32> first, d_gains, ck_off, table, d_denom, d_cov0;
    DevBuf<u64> d_out;
    TRY(first.alloc(total));
    TRY(d_gains.alloc(np));
    HIP_TRY(hipMemsetAsync(first.p, 0xff, sizeof(u32) * (size_t)total, s));
    HIP_TRY(hipMemsetAsync(d_gains.p, 0, sizeof(u32) * (size_t)np, s));
    const size_t ntab = (size_t)nc * ngu;
    std::vector<u32> h_small;                                // {0, k_0 ..}, denom, covered0: one pageable upload each
    if (nc) {
        TRY(ck_off.alloc((size_t)nc + 1));
        TRY(table.alloc(ntab));
        TRY(d_denom.alloc(ngu));
        TRY(d_cov0.alloc(ngu));
        TRY(d_out.alloc(3 * (size_t)nc));
        HIP_TRY(hipMemsetAsync(table.p, 0, sizeof(u32) * (ntab ? ntab : 1), s));
        h_small.resize((size_t)nc + 1 + 2 * (size_t)ngu);
        h_small[0] = 0;
        for (u32 j = 0; j < nc; ++j) h_small[j + 1] = (u32)checkpoints[j];
        for (u32 u = 0; u < ngu; ++u) {
            h_small[(size_t)nc + 1 + u] = (u32)denom[u];
            h_small[(size_t)nc + 1 + ngu + u] = covered0 ? (u32)covered0[u] : 0u;
        }
        HIP_TRY(hipMemcpyAsync(ck_off.p, h_small.data(), sizeof(u32) * ((size_t)nc + 1), hipMemcpyHostToDevice, s));
        if (ngu) {
            HIP_TRY(hipMemcpyAsync(d_denom.p, h_small.data() + nc + 1, sizeof(u32) * (size_t)ngu,
                                   hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_cov0.p, h_small.data() + nc + 1 + ngu, sizeof(u32) * (size_t)ngu,
                                   hipMemcpyHostToDevice, s));
        }
    }
    const dim3 blk(256);
    if (n0 && total) {
        const dim3 per_row((unsigned)div_up(n0, 256 / WAVE));
        hipLaunchKernelGGL(gn_first_kernel, per_row, blk, 0, s, (const i32 *)R0->set_id.p, (const u32 *)R0->gs.p,
                           (const u32 *)R0->ge.p, n0, ns, (const u32 *)rank.p, total, first.p);
        hipLaunchKernelGGL(gn_count_kernel, per_row, blk, 0, s, (const i32 *)R0->set_id.p, (const i32 *)R0->univ.p,
                           (const u32 *)R0->gs.p, (const u32 *)R0->ge.p, n0, ns, (const u32 *)rank.p, total,
                           (const u32 *)first.p, d_gains.p, (const u32 *)ck_off.p, nc, ngu, table.p);
        tm.launch(2);
    }
    if (nc) {
        if (ngu) {
            hipLaunchKernelGGL(gn_prefix_kernel, dim3((unsigned)div_up(ngu, 256)), blk, 0, s, table.p, nc, ngu,
                               (const u32 *)d_cov0.p);
            tm.launch(1);
        }
        hipLaunchKernelGGL(gn_reduce_kernel, dim3(nc), blk, 0, s, (const u32 *)table.p, ngu, (const u32 *)d_denom.p,
                           d_out.p);
        tm.launch(1);
    }
    HIP_TRY(hipGetLastError());
    tm.stop();
    const size_t out_bytes = sizeof(u64) * 3 * (size_t)nc, gain_bytes = sizeof(u32) * (size_t)np;
    TRY(chip_pinned_reserve(ctx, out_bytes + gain_bytes));
    if (nc) HIP_TRY(hipMemcpyAsync(ctx->h_big, d_out.p, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync((char *)ctx->h_big + out_bytes, d_gains.p, gain_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                        // (also: the pageable h_small has been read)
    memcpy(gains, (const char *)ctx->h_big + out_bytes, gain_bytes);
    const u64 *h = (const u64 *)ctx->h_big;
    for (u32 j = 0; j < nc; ++j) {
        covered_total[j] = h[3 * (size_t)j];
        const u32 wu = (u32)h[3 * (size_t)j + 1];
        worst_universe[j] = wu == GN_NONE ? -1 : (i32)wu;
        worst_covered[j] = (i64)h[3 * (size_t)j + 2];
    }
    tm.finish();
    return 0;
}
