// Bucketed row build (included by scan.hip).
//
// Turns the hit records of a scan into the cover-row table of
// SetCoverFilter._make_sets (catch/filter/set_cover_filter.py:424-453 +
// catch/utils/interval.py:288-316): per set, per universe, the union of the
// extended / clipped cover ranges, sorted by (set id, universe, start).
//
// Instead of a global radix sort of all hits (6 passes x 5 launches), hits are
// grouped by set id with one counting pass -- the producing kernel takes
// rank = atomicAdd(&bcnt[bucket], 1) per hit, the addresses are spread over
// thousands of buckets -- a scan of the bucket sizes and a scatter.  One
// wavefront per bucket then sorts its (few dozen) intervals by start in LDS
// (rank sort), merges overlapping / touching ones with wave scans and writes
// the merged rows back in place.  A second scan of the merged counts and one
// emit kernel produce the final table.  The whole build is stream-ordered; the
// host synchronises once, to learn the number of rows.
//
// When the rows go straight to the row-parallel solver (catchhip_setcover_filter,
// synchronous branch) the emit kernel is not launched: the bucket-grouped records ARE
// the table ("direct rows", catchhip_rows::rows4 in internal.h).  What the solver relies
// on: every producer files a record under its bucket's number (.w), the merge walk
// writes a bucket's mcnt[b] merged rows to its FIRST slots in start order and leaves the
// stale records behind them in place with .w == b -- so slot i is a row iff
// i - bstart[S[i].w] < mcnt[S[i].w], and when nothing merged every slot is one.  The emit
// kernel then only serves the callers that keep the table (catchhip_cover_scan) and the
// solvers that index four arrays (chip_rows_materialise).
//
// Buckets larger than BK_SMALL go to a workgroup-wide instance of the same
// code (BK_BIG); beyond that the caller falls back to the radix-sort build.

struct HitSink {
    uint4 *rec;            // per hit record {start, end, segment, bucket} (extended + clipped)
    u32 *rank;             // per hit record: rank inside its bucket, BK_NONE = no hit
    // Compact filing (seed scan): the hits of every 64 work items sit at the FRONT
    // of their 64 record slots and wcnt[d / 64] says how many there are -- a
    // wavefront's ~15 hits are 2-3 full lines of rec instead of 15 records
    // sprinkled over 8 lines, and the scatter reads nothing for the misses.
    // null: record d belongs to work item d, misses have rank BK_NONE.
    u32 *wcnt = nullptr;
    u32 *bcnt;             // per bucket: hits
    const u32 *bucket_of;  // probe -> bucket (null: the probe index itself)
    const i32 *seq_genome; // sequence -> genome (null: segments are sequences)
    u32 ext;               // cover extension
    // independent instances in one scan (catchhip_*_set_groups): a probe only
    // covers sequences of its own group; null = no groups
    const i32 *probe_group = nullptr;   // per unique probe
    const i32 *seq_group = nullptr;     // per sequence
};
#define BK_NONE 0xffffffffu
#define BK_SMALL 512       // bucket sizes one wavefront handles
#define BK_BIG 8192        // bucket sizes one workgroup handles (96 KB of LDS)

// one hit: probe p covers [gs, ge) inside sequence sq = [lo, hi)
__device__ __forceinline__ void hit_record(const HitSink &k, u32 d, u32 p, u32 gs, u32 ge, u32 sq, u32 lo, u32 hi) {
    if (k.probe_group && k.probe_group[p] != k.seq_group[sq]) { k.rank[d] = BK_NONE; return; }
    const u32 es = (gs - lo > k.ext) ? gs - k.ext : lo;
    const u32 ee = (hi - ge > k.ext) ? ge + k.ext : hi;
    const u32 b = k.bucket_of ? k.bucket_of[p] : p;
    const u32 seg = k.seq_genome ? (u32)k.seq_genome[sq] : sq;
    k.rec[d] = make_uint4(es, ee, seg, b);
    k.rank[d] = atomicAdd(&k.bcnt[b], 1u);
}

// Files the verdict of work item d.  Called by all live lanes of a wavefront
// together, lane l holding item 64 * (d / 64) + l.
__device__ __forceinline__ void hit_file(const HitSink &k, u32 d, bool hit, u32 p, u32 gs, u32 ge, u32 sq, u32 lo, u32 hi) {
    if (k.wcnt) {
        const unsigned long long hb = __ballot(hit);
        const u32 lane = d & 63u;
        if (lane == 0) k.wcnt[d >> 6] = (u32)__popcll(hb);
        if (hit) hit_record(k, (d & ~63u) + (u32)__popcll(hb & ((1ull << lane) - 1ull)), p, gs, ge, sq, lo, hi);
    } else if (hit) {
        hit_record(k, d, p, gs, ge, sq, lo, hi);
    } else {
        k.rank[d] = BK_NONE;
    }
}

// hit records from a compact hit list (tiled scan, seed-join path)
__global__ void __launch_bounds__(256)
hit_record_kernel(const u32 *__restrict__ hp, const u32 *__restrict__ hs, const u32 *__restrict__ he, u32 fixed_len,
                  u32 n, const u32 *__restrict__ seq_off, u32 nseq, HitSink k) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const u32 gs = hs[t], ge = he ? he[t] : gs + fixed_len;
    const u32 sq = find_segment(seq_off, nseq, gs);
    hit_record(k, t, hp[t], gs, ge, sq, seq_off[sq], seq_off[sq + 1]);
}

// Exclusive scan of n counts by ONE workgroup (n up to a few million: each
// thread owns a contiguous chunk).  out[n] = total; *total_out = total;
// *max_out = max(in) and, if aux, *auxmax_out = max(aux[0..n)).
__global__ void __launch_bounds__(1024)
scan1_kernel(const u32 *in, u32 *__restrict__ out, u32 n, u32 *__restrict__ total_out, u32 *__restrict__ max_out,
             const u32 *__restrict__ aux, u32 *__restrict__ auxmax_out) {
    __shared__ u32 s_part[16], s_mx[16], s_amx[16];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // any multiple of 64 threads up to 1024 (launched with 1024; measured on
    // S2 with two groups in flight: 256 or 512 threads need more dependent load
    // batches and cost 10 us per group more than 1024)
    const u32 nthreads = blockDim.x, nwaves = nthreads >> 6;
    const u32 per = (n + nthreads - 1u) / nthreads;
    const u32 lo = min(n, tid * per), hi = min(n, lo + per);
    u32 sum = 0, mx = 0, amx = 0;
    // all loads of a chunk are issued before the first use (one memory round
    // trip per SC1_R items instead of one per item)
    constexpr int SC1_R = 16;
    u32 keep[SC1_R];
#pragma unroll
    for (int j = 0; j < SC1_R; ++j) keep[j] = 0;
    for (u32 i0 = lo; i0 < hi; i0 += SC1_R) {
        u32 v[SC1_R], av[SC1_R];
#pragma unroll
        for (int j = 0; j < SC1_R; ++j) {
            const u32 i = min(i0 + j, hi - 1);
            v[j] = in[i];
            av[j] = aux ? aux[i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < SC1_R; ++j) {
            if (i0 + j < hi) { sum += v[j]; mx = max(mx, v[j]); amx = max(amx, av[j]); }
            if (i0 == lo) keep[j] = (i0 + j < hi) ? v[j] : 0u;
        }
    }
    const u32 inc = wave_incl_scan(sum, (int)lane);
    wave_max_n(mx, amx);
    if (lane == 63) s_part[wave] = inc;
    if (lane == 0) { s_mx[wave] = mx; s_amx[wave] = amx; }
    __syncthreads();
    u32 woff = 0, tot = 0, m = 0, am = 0;
    for (int w = 0; w < (int)nwaves; ++w) {
        if (w < (int)wave) woff += s_part[w];
        tot += s_part[w];
        m = max(m, s_mx[w]);
        am = max(am, s_amx[w]);
    }
    u32 run = woff + inc - sum;
#pragma unroll
    for (int j = 0; j < SC1_R; ++j) {
        if (lo + j < hi) out[lo + j] = run;
        run += keep[j];
    }
    for (u32 i0 = lo + SC1_R; i0 < hi; i0 += SC1_R) {
        u32 v[SC1_R];
#pragma unroll
        for (int j = 0; j < SC1_R; ++j)
            v[j] = in[min(i0 + j, hi - 1)];
#pragma unroll
        for (int j = 0; j < SC1_R; ++j) {
            if (i0 + j < hi) { out[i0 + j] = run; run += v[j]; }
        }
    }
    if (tid == 0) {
        out[n] = tot;
        if (total_out) *total_out = tot;
        if (max_out) *max_out = m;
        if (auxmax_out) *auxmax_out = am;
    }
}

// Larger inputs: tiles of SCT_TILE items, two launches.  scan_tiles_reduce
// writes each tile's sum (and max of aux); scan_tiles_apply lets every
// workgroup add up the sums of the tiles before its own (a few thousand
// values at most) and scan its tile.
#define SCT_THREADS 256
#define SCT_IPT 16
#define SCT_TILE (SCT_THREADS * SCT_IPT)
__global__ void __launch_bounds__(SCT_THREADS)
scan_tiles_reduce_kernel(const u32 *in, u32 n, const u32 *__restrict__ aux, u32 *__restrict__ tsum,
                         u32 *__restrict__ tamax) {
    __shared__ u32 s_sum[SCT_THREADS / 64], s_amx[SCT_THREADS / 64];
    const u32 t0 = blockIdx.x * SCT_TILE;
    u32 sum = 0, amx = 0;
#pragma unroll
    for (int j = 0; j < SCT_IPT; ++j) {
        const u32 i = t0 + j * SCT_THREADS + threadIdx.x;
        if (i < n) {
            sum += in[i];
            if (aux) amx = max(amx, aux[i]);
        }
    }
    wave_sum_max(sum, amx);
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = sum; s_amx[threadIdx.x >> 6] = amx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 a = 0, m = 0;
        for (int w = 0; w < SCT_THREADS / 64; ++w) { a += s_sum[w]; m = max(m, s_amx[w]); }
        tsum[blockIdx.x] = a;
        tamax[blockIdx.x] = m;
    }
}

__global__ void __launch_bounds__(SCT_THREADS)
scan_tiles_apply_kernel(const u32 *in, u32 *__restrict__ out, u32 n, const u32 *__restrict__ tsum,
                        const u32 *__restrict__ tamax, u32 ntiles, u32 *__restrict__ total_out,
                        u32 *__restrict__ auxmax_out) {
    __shared__ u32 s_red[SCT_THREADS / 64], s_red2[SCT_THREADS / 64], s_wsum[SCT_THREADS / 64];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // sum of the tiles before this one; the last workgroup also totals everything
    const bool is_last = blockIdx.x == ntiles - 1;
    u32 before = 0, amx = 0;
    for (u32 i = tid; i < (is_last ? ntiles : blockIdx.x); i += SCT_THREADS) {
        if (i < blockIdx.x) before += tsum[i];
        amx = max(amx, tamax[i]);
    }
    wave_sum_max(before, amx);
    if (lane == 0) { s_red[wave] = before; s_red2[wave] = amx; }
    __syncthreads();
    before = 0; amx = 0;
    for (int w = 0; w < SCT_THREADS / 64; ++w) { before += s_red[w]; amx = max(amx, s_red2[w]); }
    // thread-contiguous items: item index = t0 + tid * SCT_IPT + j
    const u32 t0 = blockIdx.x * SCT_TILE + tid * SCT_IPT;
    u32 v[SCT_IPT], sum = 0;
#pragma unroll
    for (int j = 0; j < SCT_IPT; ++j) {
        v[j] = (t0 + j < n) ? in[t0 + j] : 0u;
        sum += v[j];
    }
    const u32 inc = wave_incl_scan(sum, (int)lane);
    if (lane == 63) s_wsum[wave] = inc;
    __syncthreads();
    u32 woff = 0, tile_total = 0;
    for (int w = 0; w < SCT_THREADS / 64; ++w) { if (w < (int)wave) woff += s_wsum[w]; tile_total += s_wsum[w]; }
    u32 run = before + woff + inc - sum;
#pragma unroll
    for (int j = 0; j < SCT_IPT; ++j) {
        if (t0 + j < n) out[t0 + j] = run;
        run += v[j];
    }
    if (is_last && tid == 0) {
        out[n] = before + tile_total;
        if (total_out) *total_out = before + tile_total;
        if (auxmax_out) *auxmax_out = max(amx, tamax[blockIdx.x]);
    }
}

// hit record d -> slot bstart[bucket] + rank of the bucket-grouped arrays
__global__ void __launch_bounds__(256)
bucket_scatter_kernel(const uint4 *__restrict__ rec, const u32 *__restrict__ rank, u32 nrec_cap,
                      const u32 *__restrict__ nrec_dev, const u32 *__restrict__ bstart, uint4 *__restrict__ S,
                      const u32 *__restrict__ wcnt) {
    const u32 d = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 n = nrec_dev ? min(*nrec_dev, nrec_cap) : nrec_cap;
    if (d >= n) return;
    if (wcnt && (d & 63u) >= wcnt[d >> 6]) return;   // compact filing: past the hits of these 64 work items
    const u32 rk = rank[d];
    if (rk == BK_NONE) return;
    const uint4 r = rec[d];
    const u32 slot = bstart[r.w] + rk;
    S[slot] = r;   // one 16-byte record per hit {start, end, segment, bucket}: a single scattered write
}

// Merge walk over a bucket sorted by start (LDS arrays): one wavefront, 64
// items at a time, wave scans with a carry between chunks.  Writes the merged
// rows back at the bucket's first slots and its row count / longest row /
// total length.
__device__ __forceinline__ void bucket_merge_walk(const u32 *s_es, const u32 *s_ee, const u32 *s_sg, u32 n, u32 base,
                                                  u32 b, u32 lane, uint4 *__restrict__ S, u32 *__restrict__ mcnt,
                                                  u32 *__restrict__ blmax, unsigned long long *__restrict__ bsum,
                                                  int dedupe) {
    u32 out = 0, lmax = 0;
    unsigned long long total_len = 0;
    if (dedupe) {
        // coverage analysis (find_probe_covers_in_sequence with merge_overlapping=
        // False, catch/probe.py:1268-1270): identical ranges collapse, nothing is
        // merged.  The bucket is sorted by (start, end), so duplicates are adjacent.
        for (u32 c0 = 0; c0 < n; c0 += 64) {
            const u32 i = c0 + lane;
            const bool valid = i < n;
            const u32 es = valid ? s_es[i] : 0u, ee = valid ? s_ee[i] : 0u;
            const bool head = valid && (i == 0 || s_es[i - 1] != es || s_ee[i - 1] != ee);
            const unsigned long long hb = __ballot(head);
            if (head) {
                const u32 o = out + (u32)__popcll(hb & ((1ull << lane) - 1ull));
                S[base + o] = make_uint4(es, ee, s_sg[i], b);
                lmax = max(lmax, ee - es);
                total_len += ee - es;
            }
            out += (u32)__popcll(hb);
        }
        // (wave_sum_max of wave.h, written out here and at the end of the walk: through the helper bucket_merge_big_kernel's
        // register count moves, 40 -> 39 VGPRs)
        for (int d = 32; d > 0; d >>= 1) { lmax = max(lmax, __shfl_down(lmax, d)); total_len += __shfl_down(total_len, d); }
        if (lane == 0) { mcnt[b] = out; blmax[b] = lmax; if (bsum) bsum[b] = total_len; }
        return;
    }
    u32 c_sg = 0xffffffffu, c_max = 0, c_start = 0;   // run in progress at the end of the previous chunk
    for (u32 c0 = 0; c0 < n; c0 += 64) {
        const u32 i = c0 + lane;
        const bool valid = i < n;
        const u32 es = valid ? s_es[i] : 0u, ee = valid ? s_ee[i] : 0u;
        const u32 sg = valid ? s_sg[i] : (0xfffffffeu - lane);   // invalid lanes never combine
        // inclusive prefix max of the ends inside the segment
        u32 pm = ee;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 o_pm = __shfl_up(pm, d), o_sg = __shfl_up(sg, d);
            if ((int)lane >= d && o_sg == sg) pm = max(pm, o_pm);
        }
        if (sg == c_sg) pm = max(pm, c_max);
        // ends seen before this item in its segment
        const u32 p_pm = __shfl_up(pm, 1), p_sg = __shfl_up(sg, 1);
        bool has_prev; u32 prev;
        if (lane == 0) { has_prev = sg == c_sg; prev = c_max; }
        else { has_prev = p_sg == sg; prev = p_pm; }
        const bool head = valid && (!has_prev || es > prev);   // touching intervals merge
        // start of the run this item belongs to
        const unsigned long long hb = __ballot(head);
        const unsigned long long upto = hb & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        const int src = upto ? 63 - __builtin_clzll(upto) : 0;
        const u32 h_es = __shfl(es, src);
        const u32 rs = upto ? h_es : c_start;
        // last item of its run?
        bool last = false;
        if (valid) {
            if (i + 1 >= n) last = true;
            else last = s_sg[i + 1] != sg || s_es[i + 1] > pm;
        }
        const unsigned long long lb = __ballot(last);
        if (last) {
            const u32 o = out + (u32)__popcll(lb & ((1ull << lane) - 1ull));
            S[base + o] = make_uint4(rs, pm, sg, b);
            lmax = max(lmax, pm - rs);
            total_len += pm - rs;
        }
        out += (u32)__popcll(lb);
        const int lastlane = (int)min(63u, n - c0 - 1u);
        c_sg = __shfl(sg, lastlane); c_max = __shfl(pm, lastlane); c_start = __shfl(rs, lastlane);
    }
    for (int d = 32; d > 0; d >>= 1) { lmax = max(lmax, __shfl_down(lmax, d)); total_len += __shfl_down(total_len, d); }
    if (lane == 0) { mcnt[b] = out; blmax[b] = lmax; if (bsum) bsum[b] = total_len; }
}

// rank sort of the n <= THREADS * IPT items in the LDS arrays by (start, end, index):
// one 64-bit compare of (start << 32 | end) per pair instead of a three-level
// comparison chain (rocprofv3: ~20 VALU + SALU instructions per pair before)
template <int THREADS, int IPT>
__device__ __forceinline__ void bucket_rank_sort(u32 *s_es, u32 *s_ee, u32 *s_sg, u32 n, u32 tid) {
    unsigned long long my_k[IPT];
    u32 my_sg[IPT], rk[IPT];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const u32 i = tid + k * THREADS;
        rk[k] = 0;
        my_k[k] = i < n ? ((unsigned long long)s_es[i] << 32) | s_ee[i] : ~0ull;
        my_sg[k] = i < n ? s_sg[i] : 0u;
    }
    for (u32 j = 0; j < n; ++j) {
        const unsigned long long kj = ((unsigned long long)s_es[j] << 32) | s_ee[j];
#pragma unroll
        for (int k = 0; k < IPT; ++k)
            rk[k] += (kj < my_k[k] || (kj == my_k[k] && j < tid + k * THREADS)) ? 1u : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const u32 i = tid + k * THREADS;
        if (i < n) { s_es[rk[k]] = (u32)(my_k[k] >> 32); s_ee[rk[k]] = (u32)my_k[k]; s_sg[rk[k]] = my_sg[k]; }
    }
}

// The no-touch path of bucket_merge_kernel<.., RUNS = true> (the comment there says what it relies on): one
// wavefront, bucket of n <= 64 * NQ records given as runs rs[a] .. rs[a + 1], lane l holds records l, l + 64, ..
// in registers.  Fills s_es / s_ee, ranks every record and tests it for a touch.  Clean bucket: stores the records
// that are not at their place, the bucket's counts, and returns true.  Otherwise nothing is stored, s_sg is filled
// too and the caller takes the general path.
// BK_NT_SLOTS: the most register slots the path is built with.  With 8 (every wave bucket) the first version needed
// 133 VGPRs, 3 wavefronts per SIMD; with 4 the kernel needs 82 and runs 5 (the general path alone: 71 and 7).
// Buckets of more than 256 records take the general path; S4 has none (profiles/r10_bucket_distribution_S4.json).
#define BK_RUNS_MAX 5
#define BK_NT_SLOTS 4
// inclusive maximum over the 64 lanes, the steps of wave_incl_scan_dpp (wave.h): lanes a step does not reach see 0
__device__ __forceinline__ u32 bucket_incl_max_dpp(u32 v) {
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
    v = max(v, (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
    return v;
}
template <int NQ>
__device__ __forceinline__ bool bucket_no_touch(u32 *s_es, u32 *s_ee, u32 *s_sg, const u32 (&rs)[BK_RUNS_MAX + 1], u32 n,
                                                u32 base, u32 b, u32 lane, uint4 *__restrict__ S, u32 *__restrict__ mcnt,
                                                u32 *__restrict__ blmax, unsigned long long *__restrict__ bsum) {
    u32 es[NQ], ee[NQ], sg[NQ], rk[NQ];
    __syncthreads();   // previous bucket's merge is done with the LDS arrays
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const u32 i = lane + q * 64u;
        es[q] = ee[q] = sg[q] = 0;
        if (i < n) { const uint4 r = S[base + i]; es[q] = r.x; ee[q] = r.y; sg[q] = r.z; s_es[i] = r.x; s_ee[i] = r.y; }
    }
    __syncthreads();
    // Per run, the records that start at or before mine (`<=` on the 32-bit starts), by a search whose trip count
    // depends on the run's length alone: the loop is the wavefront's, a lane only moves its position, and the slots
    // of a lane share the steps.  My own run counts me in, so over all runs the count is my rank + 1 in a clean
    // bucket.  The last record found in a run, stepping over myself, is the one of that run that could reach me.
    bool touched = false;
#pragma unroll
    for (int q = 0; q < NQ; ++q) rk[q] = 0;
#pragma unroll
    for (int a = 0; a < BK_RUNS_MAX; ++a) {
        if (rs[a + 1] == rs[a]) continue;
        u32 pos[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) pos[q] = rs[a];
        for (u32 len = rs[a + 1] - rs[a]; len > 1;) {
            const u32 half = len >> 1;
#pragma unroll
            for (int q = 0; q < NQ; ++q) pos[q] = s_es[pos[q] + half] <= es[q] ? pos[q] + half : pos[q];
            len -= half;
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int i = (int)(lane + q * 64u);
            const u32 lo = pos[q] + (s_es[pos[q]] <= es[q] ? 1u : 0u);
            rk[q] += lo - rs[a];
            int j = (int)lo - 1;
            j -= j == i ? 1 : 0;
            const u32 near_end = s_ee[max(j, (int)rs[a])];
            if (j >= (int)rs[a] && near_end >= es[q] && (u32)i < n) touched = true;
        }
    }
    u32 lmax = 0, len_lo = 0, len_hi = 0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const u32 i = lane + q * 64u;
        rk[q] = i < n ? rk[q] - 1u : i;
        const u32 len = ee[q] - es[q];        // (the slots past the bucket hold zeros)
        lmax = max(lmax, len);
        len_lo += len & 0xffffu;
        len_hi += len >> 16;
    }
    if (__ballot(touched) != 0ull) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const u32 i = lane + q * 64u;
            if (i < n) s_sg[i] = sg[q];
        }
        return false;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const u32 i = lane + q * 64u;
        if (i < n && rk[q] != i) S[base + rk[q]] = make_uint4(es[q], ee[q], sg[q], b);
    }
    // the bucket's longest row and total length by DPP moves instead of 18 LDS permutes; the total as two sums of
    // 16-bit halves (at most 256 values each): LANE 63 holds the results
    lmax = bucket_incl_max_dpp(lmax);
    const u32 sum_lo = wave_incl_scan_dpp(len_lo), sum_hi = wave_incl_scan_dpp(len_hi);
    if (lane == 63) {
        mcnt[b] = n; blmax[b] = lmax;
        if (bsum) bsum[b] = ((unsigned long long)sum_hi << 16) + sum_lo;
    }
    return true;
}

// Sort one bucket by start, merge per segment, write the merged rows back at
// the bucket's first slots.  Instantiated with THREADS = 64: one wavefront
// per bucket (the barriers are wave-wide no-ops), rank sort of up to CAP items;
// larger buckets are listed for bucket_merge_big_kernel.
// run_cnt (key-grouped join, buckets = probes): bucket b is the concatenation of `nruns` runs of run_cnt[b *
// run_stride + a] records, EACH sorted by (start, end) -- the hits of one anchor entry in position order.  An
// item's place in the merged order is its index in its own run + the number of smaller items in the other runs,
// found by binary search in LDS: O(log n) per item where the rank sort needs O(n) (the concatenation is never
// nearly sorted, so the odd-even rounds always gave up: 20 ms per S4 step in the first version of the join).
//
// RUNS (the instance launched with run_cnt and without dedupe: the join's, hence every bucket of S4): a bucket in
// which NOTHING TOUCHES leaves the kernel as it came, only in start order -- every record is a row of its own -- so
// the permute through LDS, the walk and the write-back of records that already stand at their place are work whose
// result is known once the bucket is known to be clean.  Per item, in registers: the searches that rank it (on the
// 32-bit starts alone, `<=`) also find, in every other run, the last record that starts at or before it; the item is
// TOUCHED iff the end of one of those, or of its predecessor in its own run, is >= its start (segments ignored: a
// touch across two genomes only sends the bucket down the general path, which is exact).  Equal starts count as a
// touch (the record found has end >= its start = mine), so a clean bucket never needs a tie order.
// Why the nearest records are enough: let y start at or before x and reach it (end_y >= start_x).  y's successor y'
// in y's own run starts at or before x's place too (it is x, or the run's last record before x, or one before that),
// so start_y <= start_y' <= start_x <= end_y: y' is touched by its own predecessor and the bucket is not clean.
// Hence if no item is touched, no record reaches a later one: every prefix maximum of the ends is the predecessor's
// own end, below the next start, and the walk would open a row at every item -- mcnt = n, rows = records.
// A clean bucket stores only the records whose rank is not their place (one non-empty run: nothing); no store to S
// is issued before the verdict of the whole bucket is known, and a touched bucket then takes the general path below
// as every bucket did before (64-bit rank, ties to the earlier run, permute, walk), the stale records behind the
// merged rows included.
template <int THREADS, int CAP, bool RUNS = false>
__global__ void __launch_bounds__(THREADS)
bucket_merge_kernel(const u32 *__restrict__ bstart, u32 nb, uint4 *__restrict__ S, u32 *__restrict__ mcnt,
                    u32 *__restrict__ blmax,
                    unsigned long long *__restrict__ bsum, int dedupe, const u32 *__restrict__ run_cnt, int run_stride,
                    int nruns) {
    constexpr int IPT = CAP / THREADS;
    static_assert(!RUNS || THREADS == 64, "the no-touch path takes its verdict from one wavefront's ballot");
    __shared__ u32 s_es[CAP], s_ee[CAP], s_sg[CAP];
    const u32 tid = threadIdx.x, lane = tid & 63;
    for (u32 b = blockIdx.x; b < nb; b += gridDim.x) {
        const u32 base = bstart[b], n = bstart[b + 1] - base;
        if (n > (u32)CAP) continue;   // bucket_merge_big_kernel's
        if (n == 0) {
            if (tid == 0) { mcnt[b] = 0; blmax[b] = 0; if (bsum) bsum[b] = 0; }
            continue;
        }
        bool filled = false;   // the LDS arrays hold the bucket already
        if constexpr (RUNS) {
            if (n == 1) {   // one record: a row as it stands (a sixth of S4's buckets)
                if (lane == 0) { const uint4 r = S[base]; mcnt[b] = 1; blmax[b] = r.y - r.x; if (bsum) bsum[b] = r.y - r.x; }
                continue;
            }
            u32 rs[BK_RUNS_MAX + 1];
            rs[0] = 0;
#pragma unroll
            for (int a = 0; a < BK_RUNS_MAX; ++a) rs[a + 1] = rs[a] + (a < nruns ? run_cnt[(size_t)b * run_stride + a] : 0u);
            if (rs[BK_RUNS_MAX] == n && !dedupe && n <= 64u * BK_NT_SLOTS) {
                // as many register slots per lane as the bucket needs: 1 up to 64 records, 2 up to 128, 4 up to 256
                const bool clean =
                    n <= 64u ? bucket_no_touch<1>(s_es, s_ee, s_sg, rs, n, base, b, lane, S, mcnt, blmax, bsum)
                    : n <= 128u ? bucket_no_touch<2>(s_es, s_ee, s_sg, rs, n, base, b, lane, S, mcnt, blmax, bsum)
                                : bucket_no_touch<BK_NT_SLOTS>(s_es, s_ee, s_sg, rs, n, base, b, lane, S, mcnt, blmax, bsum);
                if (clean) continue;
                // something touches: the general path below, on the bucket as it stands in LDS
                filled = true;
            }
        }
        if (!filled) {
            __syncthreads();   // previous bucket's merge is done with the LDS arrays
            for (u32 i = tid; i < n; i += THREADS) { const uint4 r = S[base + i]; s_es[i] = r.x; s_ee[i] = r.y; s_sg[i] = r.z; }
        }
        __syncthreads();
        // rank sort by (start, end, index), with as many items per thread as the
        // bucket needs: the comparison loop is n x (items per thread) and was the
        // whole kernel (rocprofv3: 1,350 VALU + 1,600 SALU instructions per bucket of
        // ~70 hits with the fixed 8 items per thread, VALU 66 % busy)
        // ... unless the bucket arrived (nearly) in order, which is the rule on the
        // seed path: the scan walks the targets front to back with a few hundred
        // thousand seeds in flight, and two hits of one probe are usually a genome
        // or more apart, so the ranks (arrival order) follow the position up to
        // swaps of neighbours.  A few rounds of odd-even transposition (stable, like
        // the rank sort) finish such a bucket; one that is still out of order after
        // them takes the rank sort.
        // (round budget: about half of what the rank sort of a bucket of this size costs)
        bool merged_runs = false;
        if (run_cnt && n > 1) {
            u32 rs[BK_RUNS_MAX + 1];
            rs[0] = 0;
#pragma unroll
            for (int a = 0; a < BK_RUNS_MAX; ++a) rs[a + 1] = rs[a] + (a < nruns ? run_cnt[(size_t)b * run_stride + a] : 0u);
            if (rs[BK_RUNS_MAX] == n) {          // (always, unless the caller's buckets are not its probes)
                unsigned long long my_k[IPT];
                u32 my_sg[IPT], rk[IPT];
#pragma unroll
                for (int q = 0; q < IPT; ++q) {
                    const u32 i = tid + q * THREADS;
                    rk[q] = 0; my_k[q] = 0; my_sg[q] = 0;
                    if (i < n) {
                        my_k[q] = ((unsigned long long)s_es[i] << 32) | s_ee[i];
                        my_sg[q] = s_sg[i];
                        int r = 0;
#pragma unroll
                        for (int a = 1; a < BK_RUNS_MAX; ++a) r += (i >= rs[a]) ? 1 : 0;
                        u32 rank = i - rs[r];
#pragma unroll
                        for (int a = 0; a < BK_RUNS_MAX; ++a) {
                            if (a == r || rs[a + 1] == rs[a]) continue;
                            // items of run a that come before mine: key < mine, or == mine in an earlier run
                            u32 lo = rs[a], hi = rs[a + 1];
                            while (lo < hi) {
                                const u32 mid = (lo + hi) >> 1;
                                const unsigned long long km = ((unsigned long long)s_es[mid] << 32) | s_ee[mid];
                                if (km < my_k[q] || (a < r && km == my_k[q])) lo = mid + 1; else hi = mid;
                            }
                            rank += lo - rs[a];
                        }
                        rk[q] = rank;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < IPT; ++q) {
                    const u32 i = tid + q * THREADS;
                    if (i < n) { s_es[rk[q]] = (u32)(my_k[q] >> 32); s_ee[rk[q]] = (u32)my_k[q]; s_sg[rk[q]] = my_sg[q]; }
                }
                __syncthreads();
                merged_runs = true;
            }
        }
        const int max_rounds = merged_runs ? 0 : n <= (u32)THREADS ? 6 : n <= 2u * THREADS ? 12 : 32;
        bool dirty = !merged_runs;
        for (int round = 0; round < max_rounds && dirty; ++round) {
            u32 swapped = 0;
#pragma unroll
            for (u32 ph = 0; ph < 2; ++ph) {
                for (u32 j = 2 * tid + ph; j + 1 < n; j += 2 * THREADS) {
                    const u32 a_s = s_es[j], a_e = s_ee[j], b_s = s_es[j + 1], b_e = s_ee[j + 1];
                    if ((((unsigned long long)a_s << 32) | a_e) > (((unsigned long long)b_s << 32) | b_e)) {
                        const u32 a_g = s_sg[j], b_g = s_sg[j + 1];
                        s_es[j] = b_s; s_ee[j] = b_e; s_sg[j] = b_g;
                        s_es[j + 1] = a_s; s_ee[j + 1] = a_e; s_sg[j + 1] = a_g;
                        ++swapped;
                    }
                }
                __syncthreads();
            }
            const int nswap = __syncthreads_count(swapped ? 1 : 0);   // lanes that swapped: at most 2 pairs each per 128 items
            dirty = nswap != 0;
        }
        if (dirty) {
            if (n <= (u32)THREADS) bucket_rank_sort<THREADS, 1>(s_es, s_ee, s_sg, n, tid);
            else if (n <= 2u * THREADS) bucket_rank_sort<THREADS, 2>(s_es, s_ee, s_sg, n, tid);
            else bucket_rank_sort<THREADS, IPT>(s_es, s_ee, s_sg, n, tid);
            __syncthreads();
        }
        // merge: wavefront 0 walks the sorted bucket 64 items at a time
        if (tid < 64) bucket_merge_walk(s_es, s_ee, s_sg, n, base, b, lane, S, mcnt, blmax, bsum, dedupe);
    }
}

// Large buckets (listed by the wavefront instance): a 512-thread workgroup
// (1024 threads had to wait for a whole CU's worth of free wave slots whenever
// other groups' kernels were resident),
// bitonic sort of (start, end, segment) in dynamic LDS (3 x BK_BIG words),
// then the same merge walk.
#define BKB_THREADS 512
__global__ void __launch_bounds__(BKB_THREADS)
bucket_merge_big_kernel(const u32 *__restrict__ bstart, u32 nb, uint4 *__restrict__ S, u32 *__restrict__ mcnt,
                        u32 *__restrict__ blmax,
                        unsigned long long *__restrict__ bsum, u32 *__restrict__ overflow, int dedupe, u32 lo, u32 cap) {
    // Round 6: buckets of lo < n <= cap hits; cap = the LDS arrays' length.  Four launches -- caps 1,024 / 2,048 / 4,096 /
    // 8,192 with 12 / 24 / 48 / 96 KB of LDS: 4 / 4 / 3 / 1 workgroups per CU (until round 6 every bucket above BK_SMALL
    // took the 96-KB workgroup: S5's probes with 513-2,048 hits -- most of its large buckets -- sorted one per CU) -- and a
    // compare-exchange per THREAD and stage (pair t of the stage: i = 2t - (t & (j - 1)), partner i + j) instead of a
    // look at every element with half of them idle.
    extern __shared__ u32 s_dyn[];
    __shared__ u32 s_list[1024], s_nlist;
    u32 *s_es = s_dyn, *s_ee = s_dyn + cap, *s_sg = s_dyn + 2 * cap;
    const u32 tid = threadIdx.x, lane = tid & 63;
    // every workgroup looks at chunks of 1024 buckets and keeps the large ones
    for (u32 c0 = blockIdx.x * 1024u; c0 < nb; c0 += gridDim.x * 1024u) {
      __syncthreads();
      if (tid == 0) s_nlist = 0;
      __syncthreads();
      for (u32 q = tid; q < 1024u; q += BKB_THREADS) {
        const u32 b = c0 + q;
        if (b < nb) {
            const u32 n = bstart[b + 1] - bstart[b];
            if (n > (u32)BK_BIG) { if (cap == (u32)BK_BIG) { mcnt[b] = 0; blmax[b] = 0; if (bsum) bsum[b] = 0; *overflow = 1u; } }
            else if (n > lo && n <= cap) s_list[atomicAdd(&s_nlist, 1u)] = b;
        }
      }
      __syncthreads();
      const u32 nwork = s_nlist;
      for (u32 wk = 0; wk < nwork; ++wk) {
        const u32 b = s_list[wk];
        const u32 base = bstart[b], n = bstart[b + 1] - base;   // lo < n <= cap
        u32 N = 1024;
        while (N < n) N <<= 1;
        __syncthreads();   // previous bucket's merge is done with the LDS arrays
        for (u32 i = tid; i < N; i += BKB_THREADS) {
            const bool v = i < n;
            const uint4 r = v ? S[base + i] : make_uint4(0xffffffffu, 0u, 0xffffffffu, 0u);   // padding sorts to the end
            s_es[i] = r.x; s_ee[i] = r.y; s_sg[i] = r.z;
        }
        __syncthreads();
        for (u32 k = 2; k <= N; k <<= 1) {
            for (u32 j = k >> 1; j > 0; j >>= 1) {
                for (u32 t = tid; t < (N >> 1); t += BKB_THREADS) {
                    const u32 i = 2u * t - (t & (j - 1u)), p = i + j;
                    const u32 a = s_es[i], c = s_es[p];
                    const u32 ae = s_ee[i], ce = s_ee[p];
                    const bool up = (i & k) == 0;
                    const bool gt = a > c || (a == c && ae > ce), lt = a < c || (a == c && ae < ce);
                    if (up ? gt : lt) {
                        s_es[i] = c; s_es[p] = a;
                        s_ee[i] = ce; s_ee[p] = ae;
                        const u32 g0 = s_sg[i]; s_sg[i] = s_sg[p]; s_sg[p] = g0;
                    }
                }
                __syncthreads();
            }
        }
        if (tid < 64) bucket_merge_walk(s_es, s_ee, s_sg, n, base, b, lane, S, mcnt, blmax, bsum, dedupe);
      }
    }
}

// final table: row r of bucket b (found through the scanned merged counts)
__global__ void __launch_bounds__(256)
rows_emit_kernel(const u32 *__restrict__ rstart, u32 nb, const u32 *__restrict__ bstart,
                 const i32 *__restrict__ bucket_set, const uint4 *__restrict__ S, u32 nrows_cap,
                 const u32 *__restrict__ nrows_dev,
                 i32 *__restrict__ o_set, i32 *__restrict__ o_univ, u32 *__restrict__ o_gs, u32 *__restrict__ o_ge,
                 const u32 *__restrict__ nhits_dev, int nothing_merged) {
    // Nothing merged anywhere (as many rows as hits -- the rule when a probe covers a genome once): every
    // bucket still fills its slots, row r IS record r of S and carries its bucket: a plain transform.
    if (nothing_merged > 0 || (nothing_merged < 0 && nhits_dev && nrows_dev && *nhits_dev == *nrows_dev)) {
        const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
        const u32 nrows = nrows_dev ? min(*nrows_dev, nrows_cap) : nrows_cap;
        if (r >= nrows) return;
        const uint4 row = S[r];
        o_set[r] = bucket_set ? bucket_set[row.w] : (i32)row.w;
        o_univ[r] = (i32)row.z;
        o_gs[r] = row.x;
        o_ge[r] = row.y;
        return;
    }
    // The bucket of a row = the last bucket with rstart[b] <= r (empty buckets
    // share their successor's offset).  A binary search over all buckets per row
    // was 23 dependent loads per row (10 ms per S4 step); the workgroup finds the
    // bucket of its FIRST row once and stages the next 256 offsets in LDS, where
    // almost every row of the workgroup finds its bucket in 8 steps.
    __shared__ u32 s_rs[257], s_lo0;
    const u32 r0 = blockIdx.x * blockDim.x;
    const u32 r = r0 + threadIdx.x;
    const u32 nrows = nrows_dev ? min(*nrows_dev, nrows_cap) : nrows_cap;
    if (r0 >= nrows) return;
    if (threadIdx.x == 0) {
        u32 lo = 0, hi = nb;
        while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (rstart[mid] <= r0) lo = mid; else hi = mid; }
        s_lo0 = lo;
    }
    __syncthreads();
    const u32 lo0 = s_lo0;
    for (u32 q = threadIdx.x; q < 257; q += blockDim.x) s_rs[q] = lo0 + q <= nb ? rstart[min(lo0 + q, nb)] : 0xffffffffu;
    __syncthreads();
    if (r >= nrows) return;
    u32 lo, hi;
    if (s_rs[256] > r) {           // inside the staged window
        lo = 0; hi = 256;
        while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (s_rs[mid] <= r) lo = mid; else hi = mid; }
        lo += lo0;
    } else {                       // a long run of empty buckets: the full search
        lo = lo0; hi = nb;
        while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (rstart[mid] <= r) lo = mid; else hi = mid; }
    }
    const u32 src = bstart[lo] + (r - rstart[lo]);
    o_set[r] = bucket_set ? bucket_set[lo] : (i32)lo;
    const uint4 row = S[src];
    o_univ[r] = (i32)row.z;
    o_gs[r] = row.x;
    o_ge[r] = row.y;
}
