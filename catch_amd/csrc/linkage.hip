// Average-linkage clustering of the clustering pre-step's `hierarchical` method, on the device.
//
// Replaces, for `--cluster-and-design-separately` (catch/utils/cluster.py:197-232):
//   * scipy.cluster.hierarchy.linkage(dist_matrix, method="average"): SciPy's nearest-neighbour chain over the
//     condensed matrix converted to float64 (scipy/cluster/_hierarchy.pyx nn_chain, then a stable sort of the merges
//     by height and a union-find relabelling);
//   * scipy.cluster.hierarchy.fcluster(linkage, threshold, criterion="distance") (_hierarchy.pyx
//     get_max_dist_for_each_cluster + cluster_monocrit).
// The signature distances take only N + 1 distinct values, so ties are the normal case and SciPy's tie rules decide
// the clusters; they are reproduced exactly:
//   - the chain starts from the lowest live index;
//   - the nearest neighbour of the chain's top x is the lowest index attaining the minimum of row x, unless the
//     entry below the top attains it too: then it is that entry (and the two merge);
//   - the merged pair keeps the larger index; D[i][y] = (nx * D[i][x] + ny * D[i][y]) / (nx + ny) in float64 with
//     the products, the sum and the quotient each rounded on its own (no fused multiply-add).
//
// Kernels:
//   linkage_init_sigs_kernel       the tile walk of sig_pairs_kernel; writes the FULL square float64 matrix D[n][n]
//   linkage_init_condensed_kernel  (both triangles, +inf on the diagonal) from signatures + lut, or from a float32
//                                  condensed matrix (raising a flag when an entry is not finite)
//   linkage_nn_chain_kernel        ONE workgroup, persistent over the whole run: n - 1 dependent merges and at most
//                                  3 (n - 1) dependent row scans.  A scan is an argmin over one contiguous row of D
//                                  (8 n bytes): a dead cluster's column holds +inf, so there is no liveness test.  A
//                                  merge rewrites row y and column y and puts +inf into column x.  Everything is
//                                  ordered by __syncthreads(); no other workgroup exists, nothing spins on memory.
//                                  (A grid-wide barrier per step would cost tens of microseconds, more than the scan.)
// Host part (this file, like components.hip): sort, relabel, maximum heights, flat clusters.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "internal.h"

#define LK_THREADS 1024
#define LK_WAVES (LK_THREADS / WAVE)
#define LK_NONE 0xffffffffu

__global__ __launch_bounds__(256) void linkage_init_sigs_kernel(const u32 *__restrict__ sig, u32 nseq, u32 N, u32 T,
                                                                const float *__restrict__ lut, double *__restrict__ D) {
    extern __shared__ u32 s_ab[];
    const u32 bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;   // upper triangle of tiles only: a pair writes both of its entries
    u32 *s_i = s_ab, *s_j = s_ab + (size_t)T * N;
    const u32 i0 = bi * T, j0 = bj * T;
    for (u32 t = threadIdx.x; t < T * N; t += blockDim.x) {
        const u32 r = t / N, c = t - r * N;
        s_i[t] = (i0 + r < nseq) ? sig[(size_t)(i0 + r) * N + c] : 0;
        s_j[t] = (j0 + r < nseq) ? sig[(size_t)(j0 + r) * N + c] : 0;
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < T * T; t += blockDim.x) {
        const u32 li = t / T, lj = t - li * T;
        const u64 i = i0 + li, j = j0 + lj;
        if (i > j || j >= nseq) continue;
        if (i == j) { D[i * nseq + i] = __builtin_inf(); continue; }
        const u32 *pa = s_i + (size_t)li * N, *pb = s_j + (size_t)lj * N;
        const u32 common = walk_common(
            N, [&](u32 x) { return pa[x]; }, [&](u32 x) { return pb[x]; });
        const double v = (double)lut[common];
        D[i * nseq + j] = v;
        D[j * nseq + i] = v;
    }
}

__global__ __launch_bounds__(256) void linkage_init_condensed_kernel(const float *__restrict__ cond, u32 n,
                                                                     double *__restrict__ D, u32 *__restrict__ bad) {
    const u64 total = (u64)n * n;
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (u64)gridDim.x * blockDim.x) {
        const u64 i = t / n, j = t - i * n;
        if (i == j) { D[t] = __builtin_inf(); continue; }
        const u64 a = i < j ? i : j, b = i < j ? j : i;
        // condensed index of (a, b), a < b (cluster.py:94-99)
        const float v = cond[a * (u64)n - a * (a + 1) / 2 + (b - a - 1)];
        if (!(fabsf(v) < __builtin_inff())) bad[0] = 1u;      // NaN or +-inf
        D[t] = (double)v;
    }
}

// err[0]: 0 = n - 1 merges recorded; 1 = the chain would exceed n entries; 2 = the scan budget ran out;
// 3 = a row without a finite entry; 4 = no live cluster to start a chain from
__global__ __launch_bounds__(LK_THREADS) void linkage_nn_chain_kernel(double *D, u32 n, u32 *size, u32 *chain,
                                                                     double *merges, u32 *err) {
#pragma clang fp contract(off)
    __shared__ double s_v[LK_WAVES], s_dprev;
    __shared__ u32 s_i[LK_WAVES], s_x, s_prev, s_stop, s_merge, s_ma, s_mb, s_nx, s_ny;
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const double INF = __builtin_inf();
    for (u32 i = tid; i < n; i += LK_THREADS) size[i] = 1u;
    // thread 0 alone reads and writes size[] and chain[] from here on, and owns these counters
    u32 chain_len = 0, first_live = 0, k = 0;
    if (tid == 0) {
        chain[0] = 0; chain_len = 1;
        s_x = 0; s_prev = LK_NONE; s_stop = 0; s_merge = 0;
    }
    __syncthreads();
    const u64 max_scans = 3ull * n;
    for (u64 scan = 0; scan < max_scans; ++scan) {
        const u32 x = s_x, prev = s_prev;
        const double *row = D + (size_t)x * n;
        double bv = INF;
        u32 bi = LK_NONE;
        // ascending i with a strict comparison: the lowest index among this lane's minima
#pragma unroll 4
        for (u32 i = tid; i < n; i += LK_THREADS) {
            const double v = row[i];
            if (i == prev) s_dprev = v;
            if (v < bv) { bv = v; bi = i; }
        }
        // lexicographic (value, index) minimum of the wavefront ...
        for (int off = 32; off; off >>= 1) {
            const double ov = __shfl_down(bv, off, WAVE);
            const u32 oi = __shfl_down(bi, off, WAVE);
            if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { s_v[wave] = bv; s_i[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            // ... and of the workgroup
            double mv = s_v[0];
            u32 mi = s_i[0];
            for (int w = 1; w < LK_WAVES; ++w) {
                const double ov = s_v[w];
                const u32 oi = s_i[w];
                if (ov < mv || (ov == mv && oi < mi)) { mv = ov; mi = oi; }
            }
            if (!(mv < INF)) { err[0] = 3u; s_stop = 1u; }
            else if (prev != LK_NONE && s_dprev <= mv) {
                // the entry below the top is a nearest neighbour of the top: merge the two
                const u32 a = x < prev ? x : prev, b = x < prev ? prev : x;
                const u32 nx = size[a], ny = size[b];
                double *m = merges + (size_t)k * 4;
                m[0] = (double)a; m[1] = (double)b; m[2] = s_dprev; m[3] = (double)(nx + ny);
                size[a] = 0u; size[b] = nx + ny;
                s_ma = a; s_mb = b; s_nx = nx; s_ny = ny; s_merge = 1u;
                chain_len -= 2;
                ++k;
                if (k == n - 1) s_stop = 2u;
                else {
                    if (chain_len == 0) {
                        while (first_live < n && size[first_live] == 0u) ++first_live;
                        if (first_live >= n) { err[0] = 4u; s_stop = 1u; first_live = 0; }
                        chain[0] = first_live; chain_len = 1;
                    }
                    s_x = chain[chain_len - 1];
                    s_prev = chain_len >= 2 ? chain[chain_len - 2] : LK_NONE;
                }
            } else if (chain_len >= n) { err[0] = 1u; s_stop = 1u; }
            else {
                chain[chain_len++] = mi;
                s_prev = x; s_x = mi; s_merge = 0u;
            }
        }
        __syncthreads();
        if (s_stop) break;
        if (s_merge) {
            const u32 a = s_ma, b = s_mb;
            const double nx = (double)s_nx, ny = (double)s_ny, nxy = (double)(s_nx + s_ny);
            const double *ra = D + (size_t)a * n;
            double *rb = D + (size_t)b * n;
            for (u32 i = tid; i < n; i += LK_THREADS) {
                if (i == b) continue;
                const double db = rb[i];
                if (!(db < INF)) continue;          // a dead cluster: its entries are +inf already
                // (i == a: D[a][a] is +inf, so row b and column b get +inf at a, and a's column is closed below)
                const double v = __ddiv_rn(__dadd_rn(__dmul_rn(nx, ra[i]), __dmul_rn(ny, db)), nxy);
                rb[i] = v;
                D[(size_t)i * n + b] = v;
                D[(size_t)i * n + a] = INF;
            }
            __syncthreads();
        }
    }
    if (tid == 0 && k != n - 1 && err[0] == 0u) err[0] = 2u;
}

// ---- host part ----------------------------------------------------------------------------------------------------
// merges[(n - 1) * 4] = (x, y, height, size) in the order the chain produced them -> labels[n]: SciPy's 1-based flat
// cluster numbers at `threshold`; sorted[(n - 1) * 4] (may be null): the linkage matrix as SciPy returns it
static int linkage_finish(i64 n, const double *merges, double threshold, i32 *labels, double *sorted) {
    if (n == 1) { labels[0] = 1; return 0; }
    const i64 m = n - 1;
    // a stable sort by height (linkage: np.argsort(Z[:, 2], kind="mergesort"))
    std::vector<i64> order((size_t)m);
    std::iota(order.begin(), order.end(), (i64)0);
    std::stable_sort(order.begin(), order.end(), [&](i64 p, i64 q) { return merges[p * 4 + 2] < merges[q * 4 + 2]; });
    // union-find relabelling (_hierarchy.pyx label): merge k creates node n + k from the current roots, smaller first
    std::vector<i64> parent((size_t)(2 * n - 1), -1), count((size_t)(2 * n - 1), 1);
    std::vector<double> Z((size_t)m * 4);
    auto find = [&](i64 v) {
        i64 r = v;
        while (parent[r] >= 0) r = parent[r];
        while (parent[v] >= 0) { const i64 nx = parent[v]; parent[v] = r; v = nx; }
        return r;
    };
    for (i64 k = 0; k < m; ++k) {
        const double *src = merges + order[k] * 4;
        if (!(src[0] >= 0 && src[0] < (double)n && src[1] >= 0 && src[1] < (double)n) || std::isnan(src[2])) {
            chip_set_error("linkage: merge %lld is not a pair of points", (long long)order[k]);
            return CATCHHIP_EINVAL;
        }
        i64 a = find((i64)src[0]), b = find((i64)src[1]);
        if (a == b) {
            chip_set_error("linkage: merge %lld joins a cluster with itself", (long long)order[k]);
            return CATCHHIP_EINVAL;
        }
        if (a > b) std::swap(a, b);
        parent[a] = parent[b] = n + k;
        count[n + k] = count[a] + count[b];
        Z[k * 4 + 0] = (double)a; Z[k * 4 + 1] = (double)b; Z[k * 4 + 2] = src[2]; Z[k * 4 + 3] = (double)count[n + k];
    }
    if (sorted) memcpy(sorted, Z.data(), sizeof(double) * Z.size());
    // MD[k] = the largest height in the subtree of node n + k (children have smaller numbers)
    std::vector<double> MD((size_t)m);
    for (i64 k = 0; k < m; ++k) {
        double v = Z[k * 4 + 2];
        for (int c = 0; c < 2; ++c) {
            const i64 ch = (i64)Z[k * 4 + c];
            if (ch >= n && MD[ch - n] > v) v = MD[ch - n];
        }
        MD[k] = v;
    }
    // fcluster(criterion="distance") = cluster_monocrit: an iterative walk from the root, the left non-leaf child
    // first, then the right one; a node's leaf children are numbered when the walk leaves the node
    std::vector<i64> stack((size_t)n);
    std::vector<u8> visited((size_t)(2 * n - 1), 0);
    i64 depth = 0, leader = -1;
    i32 nclusters = 0;
    stack[0] = 2 * n - 2;
    while (depth >= 0) {
        const i64 root = stack[depth] - n;
        const i64 lc = (i64)Z[root * 4 + 0], rc = (i64)Z[root * 4 + 1];
        if (leader == -1 && MD[root] <= threshold) { leader = root; ++nclusters; }
        if (lc >= n && !visited[lc]) { visited[lc] = 1; stack[++depth] = lc; continue; }
        if (rc >= n && !visited[rc]) { visited[rc] = 1; stack[++depth] = rc; continue; }
        if (lc < n) { if (leader == -1) ++nclusters; labels[lc] = nclusters; }
        if (rc < n) { if (leader == -1) ++nclusters; labels[rc] = nclusters; }
        if (leader == root) leader = -1;
        --depth;
    }
    return 0;
}

extern "C" int catchhip_linkage_labels(int64_t n, const double *merges, double threshold, int32_t *labels,
                                       double *sorted) {
    ARG_CHECK(n >= 1 && n < ((i64)1 << 31) && labels && (n == 1 || merges) && !std::isnan(threshold));
    return linkage_finish(n, merges, threshold, labels, sorted);
}

// whether the float64 square matrix of n points (8 n^2 bytes) takes at most half of what the device has free right
// now (plus this library's idle cache, which an allocation returns to the driver first)
extern "C" int catchhip_linkage_fits(catchhip_ctx *ctx, int64_t n, int32_t *fits) {
    ARG_CHECK(ctx && fits && n >= 0);
    HIP_TRY(hipSetDevice(ctx->device));
    size_t fr = 0, tot = 0;
    HIP_TRY(hipMemGetInfo(&fr, &tot));
    int64_t st[4] = {0, 0, 0, 0};
    (void)catchhip_pool_stats(st);
    const double idle = st[2] > 0 ? (double)st[2] : 0.0;
    *fits = (n < ((i64)1 << 31) && 8.0 * (double)n * (double)n <= 0.5 * ((double)fr + idle)) ? 1 : 0;
    return 0;
}

// the chain over a filled matrix, then the host part
static int linkage_run(catchhip_ctx *ctx, u32 n, DevBuf<double> &D, PhaseTimer &tm, double threshold, i32 *labels,
                       double *merges_out) {
    hipStream_t st = ctx->stream;
    DevBuf<u32> d_size, d_chain, d_err;
    DevBuf<double> d_merges;
    TRY(d_size.alloc(n));
    TRY(d_chain.alloc((size_t)n + 1));
    TRY(d_err.alloc(4));
    TRY(d_merges.alloc((size_t)(n - 1) * 4));
    HIP_TRY(hipMemsetAsync(d_err.p, 0, sizeof(u32) * 4, st));
    hipLaunchKernelGGL(linkage_nn_chain_kernel, dim3(1), dim3(LK_THREADS), 0, st, D.p, n, d_size.p, d_chain.p,
                       d_merges.p, d_err.p);
    tm.launch(1);
    HIP_TRY(hipGetLastError());
    std::vector<double> h_merges((size_t)(n - 1) * 4);
    u32 h_err[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h_merges.data(), d_merges.p, sizeof(double) * h_merges.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_err, d_err.p, sizeof(h_err), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    tm.finish();
    if (h_err[0]) {
        chip_set_error("linkage: the nearest-neighbour chain stopped (%s)",
                       h_err[0] == 1 ? "chain longer than n" : h_err[0] == 2 ? "more than 3 n row scans"
                       : h_err[0] == 3 ? "a row without a finite distance" : "no live cluster");
        return CATCHHIP_EINVAL;
    }
    return linkage_finish((i64)n, h_merges.data(), threshold, labels, merges_out);
}

extern "C" int catchhip_sigs_linkage_average(catchhip_ctx *ctx, const catchhip_sigs *S, const float *lut,
                                             double threshold, int32_t *labels, double *merges) {
    ARG_CHECK(ctx && S && S->ctx == ctx && lut && labels && S->nseq >= 1 && !std::isnan(threshold));
    const u32 n = S->nseq;
    for (u32 c = 0; c <= S->N; ++c)
        if (!std::isfinite(lut[c])) {
            chip_set_error("linkage: the distance of %u common values is not finite", c);
            return CATCHHIP_EINVAL;
        }
    if (n == 1) { labels[0] = 1; return 0; }
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<double> D;
    DevBuf<float> d_lut;
    TRY(D.alloc((size_t)n * n));
    TRY(d_lut.alloc((size_t)S->N + 1));
    HIP_TRY(hipMemcpyAsync(d_lut.p, lut, sizeof(float) * ((size_t)S->N + 1), hipMemcpyHostToDevice, st));
    // both signature tiles of a workgroup live in LDS (<= 48 KB), as in catchhip_sigs_condensed
    u32 T = 32;
    while (T > 4 && sizeof(u32) * 2 * (size_t)T * S->N > 48 * 1024) T >>= 1;
    const u32 nt = (n + T - 1) / T;
    ARG_CHECK(nt <= 65535);
    PhaseTimer tm(ctx, PHASE_NDF);
    hipLaunchKernelGGL(linkage_init_sigs_kernel, dim3(nt, nt), dim3(256), sizeof(u32) * 2 * (size_t)T * S->N, st,
                       (const u32 *)S->sig.p, n, S->N, T, (const float *)d_lut.p, D.p);
    tm.launch(1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));      // (lut is read by its copy until here)
    return linkage_run(ctx, n, D, tm, threshold, labels, merges);
}

extern "C" int catchhip_linkage_average(catchhip_ctx *ctx, int64_t n64, const float *condensed, double threshold,
                                        int32_t *labels, double *merges) {
    ARG_CHECK(ctx && labels && n64 >= 1 && n64 < ((i64)1 << 31) && (n64 == 1 || condensed) && !std::isnan(threshold));
    const u32 n = (u32)n64;
    if (n == 1) { labels[0] = 1; return 0; }
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t npairs = (size_t)n * (n - 1) / 2;
    DevBuf<double> D;
    DevBuf<float> d_cond;
    DevBuf<u32> d_bad;
    TRY(D.alloc((size_t)n * n));
    TRY(d_cond.alloc(npairs));
    TRY(d_bad.alloc(1));
    HIP_TRY(hipMemsetAsync(d_bad.p, 0, sizeof(u32), st));
    HIP_TRY(hipMemcpyAsync(d_cond.p, condensed, sizeof(float) * npairs, hipMemcpyHostToDevice, st));
    PhaseTimer tm(ctx, PHASE_NDF);
    const u64 total = (u64)n * n;
    const unsigned blocks = (unsigned)std::min<u64>((total + 255) / 256, (u64)ctx->num_cus * 16);
    hipLaunchKernelGGL(linkage_init_condensed_kernel, dim3(blocks), dim3(256), 0, st, (const float *)d_cond.p, n, D.p,
                       d_bad.p);
    tm.launch(1);
    HIP_TRY(hipGetLastError());
    u32 h_bad = 0;
    HIP_TRY(hipMemcpyAsync(&h_bad, d_bad.p, sizeof(u32), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));      // (the caller's matrix is read by its copy until here)
    if (h_bad) {
        tm.finish();
        chip_set_error("linkage: the condensed distance matrix must contain only finite values");
        return CATCHHIP_EINVAL;
    }
    return linkage_run(ctx, n, D, tm, threshold, labels, merges);
}
