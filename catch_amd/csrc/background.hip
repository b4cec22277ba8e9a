// Background k-mer screen (not in the reference; catch_amd/filter/background_filter.py defines the rule and is its
// oracle): a candidate is dropped when more than H of its k-mers occur, as they are or reverse-complemented, in a
// background (a host genome, rRNA, a vector), on the device's candidate list, before the near-duplicate filter and the
// set cover like the pre-filters of prefilter.hip and thermo.hip.
//
// Code of a k-mer: 2 bits per character, (c >> 1) & 3 ('A' 0, 'C' 1, 'T' 2, 'G' 3), the first character in the most
// significant of the 2K bits of a u64; the complement of a code is code ^ 2, and canonical(w) = the smaller of code(w)
// and code(revcomp(w)), unsigned.  Both are rolled: fwd = ((fwd << 2) | c) & mask, rc = (rc >> 2) | ((c ^ 2) << (2K - 2)),
// next to the length of the run of bases that ends here; from run >= K on the two registers hold exactly the last K
// characters (K shifts push everything older out, whatever it was).  K = 32 fills the 64 bits: the mask is all ones
// (made on the host by a comparison, not by a shift of 64) and 2K - 2 = 62.
//
// The index (catchhip_kmer_index): the sorted distinct canonical codes of the background's valid k-mers, and a prefix
// directory dir[p] = index of the first code whose top P bits are >= p (2^P + 1 entries, dir[2^P] = n_unique), with
// P = clamp(ceil(log2(n_unique)), 8, min(2K, 30)): a bucket holds about one code.  Built with the scan and the sort of
// primitives.hip: kmer_emit_kernel counts, then writes, the canonical code of every valid position (a thread per
// BG_CHUNK end positions, K - 1 bytes of run-up), chip_radix_sort_pairs sorts on 2K key bits (its 4-byte values are
// dead weight here), a flag / scan / compact pass makes the list distinct.  codes and dir are plain hipMalloc blocks
// owned by the index, not by a context's block cache: every context of the device may read them, and they outlive the
// context that built them.
//
// background_flag_kernel: one thread per unique candidate, the rows staged (stage.h), one pass over its L bytes.  Per
// byte the rolling update (stage.h: KmerRoll); from run >= K on one look-up: dir[p] and dir[p + 1] (one gather of two
// neighbouring words), then the bucket -- halved while it is longer than 4, then compared one by one.  Counting:
// BG_WORDS 64-bit counters per workgroup in LDS behind the rows -- the 256 bins of hits, then "dropped".  Bin 0 and
// "dropped" are one address each for most threads, so they are summed over the wave first and added once per wave; the
// other bins take LDS atomics.  After a barrier the counters go to one of BG_SLOTS copies in global memory (stage.h:
// the totals).  No thread returns before the barrier.
//
// Mismatches (catchhip_kmer_index_create_tolerant, mismatches = M in 1, 2, K >= 8 (M + 1)): a valid k-mer hits iff some
// code of the index lies within M characters of fwd or of rc.  Block b = 0 .. M of a k-mer is its characters
// [s_b, s_(b+1)), s_b = floor(b K / (M + 1)); two k-mers within M mismatches agree in one block.  The index then holds
// M + 1 VIEWS: view 0 is codes / dir as above, view b the same codes rotated left by 2 s_b bits inside their 2K bits
// (block b leads), sorted again, with a directory of P_b = clamp(ceil(log2(n_unique)), 8, min(2 (s_(b+1) - s_b), 30))
// bits -- never finer than the block (view 0's P is capped the same way), so ONE bucket holds every code that agrees
// with a query in block b.  kmer_rotate_kernel, chip_radix_sort_pairs and kmer_dir_kernel build a view: no second emit,
// no second distinct pass (a rotation is a bijection).  background_flag_tolerant_kernel is background_flag_kernel with
// kmer_lookup.h's tolerant look-up; an index with M = 0 launches background_flag_kernel as before.
#include "internal.h"
#include "wave.h"
#include "stage.h"
#include "rule_host.h"
#include "kmer_lookup.h"

#define BG_BINS 256u
#define BG_WORDS 257u                // the bins, dropped
#define BG_SLOTS 64u
#define BG_SLOT_WORDS 272u           // 17 whole 128-byte lines
#define BG_EXTRA_BYTES (BG_WORDS * 8u)
#define BG_CHUNK 64u                 // end positions per thread of the emit kernel
#define BG_MAX_BYTES 0xfffff000ull   // the scans count in 32 bits

// ---- the index --------------------------------------------------------------------------------------------------
// WRITE = false: cnt[chunk] = valid k-mers that END in the chunk's positions; WRITE = true: their canonical codes from
// keys[at[chunk]] on.  A k-mer never spans two records: the run of bases starts again at every record start.
template <bool WRITE>
__global__ void __launch_bounds__(256)
kmer_emit_kernel(const u8 *__restrict__ bytes, const u32 *__restrict__ off, u32 nseq, u32 total, u32 nchunks, u32 K,
                 u64 mask, u32 rc_shift, u32 *__restrict__ cnt, const u32 *__restrict__ at, u64 *__restrict__ keys) {
    const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    const u64 e0 = (u64)c * BG_CHUNK;
    const u32 e1 = e0 + BG_CHUNK < (u64)total ? (u32)(e0 + BG_CHUNK) : total;
    const u32 w0 = e0 >= K - 1u ? (u32)e0 - (K - 1u) : 0u;
    u32 rec = find_segment(off, nseq, w0);
    u32 next = off[rec + 1];
    u64 fwd = 0, rc = 0;
    u32 run = 0, made = 0;
    const u32 base = WRITE ? at[c] : 0u;
    for (u32 j = w0; j < e1; ++j) {
        while (j >= next) { ++rec; next = off[rec + 1]; run = 0; }     // (j < total = off[nseq]: rec stays below nseq)
        const u8 ch = bytes[j];
        const u64 code = (ch >> 1) & 3u;
        fwd = ((fwd << 2) | code) & mask;
        rc = (rc >> 2) | ((code ^ 2ull) << rc_shift);
        run = is_base(ch) ? run + 1u : 0u;
        if (run >= K && j >= e0) {
            if (WRITE) keys[base + made] = fwd < rc ? fwd : rc;
            ++made;
        }
    }
    if (!WRITE) cnt[c] = made;
}

__global__ void __launch_bounds__(256)
kmer_head_kernel(const u64 *__restrict__ keys, u32 n, u32 *__restrict__ flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(256)
kmer_compact_kernel(const u64 *__restrict__ keys, const u32 *__restrict__ flag, const u32 *__restrict__ at, u32 n,
                    u64 *__restrict__ codes) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flag[i]) codes[at[i]] = keys[i];
}

// dir[p] = i for every prefix p above code i - 1's and up to code i's (i = n: up to 2^P): each entry written once
__global__ void __launch_bounds__(256)
kmer_dir_kernel(const u64 *__restrict__ codes, u32 n, u32 shift, u32 nprefix, u32 *__restrict__ dir) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const u32 first = i == 0 ? 0u : (u32)(codes[i - 1] >> shift) + 1u;
    const u32 last = i == n ? nprefix : (u32)(codes[i] >> shift);
    for (u32 p = first; p <= last; ++p) dir[p] = i;
}

// view b of a tolerant index, unsorted: every code rotated left by rot bits (0 < rot < bits) inside its `bits` bits
__global__ void __launch_bounds__(256)
kmer_rotate_kernel(const u64 *__restrict__ codes, u32 n, u32 rot, u32 bits, u64 mask, u64 *__restrict__ out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = ((codes[i] << rot) | (codes[i] >> (bits - rot))) & mask;
}

// the directory of one view: P = clamp(ceil(log2 n), 8, min(pcap, 30)) bits over the sorted codes (pcap >= 8)
static int kmer_view_dir(catchhip_ctx *ctx, const u64 *codes, u32 n, u32 K, u32 pcap, u32 *P_out, u32 **dir_out) {
    int P = ceil_log2_u64(n);
    const int pmax = (int)pcap < 30 ? (int)pcap : 30;
    P = P < 8 ? 8 : P > pmax ? pmax : P;
    *P_out = (u32)P;
    const u32 nprefix = (u32)1 << P;
    HIP_TRY(hipMalloc((void **)dir_out, sizeof(u32) * ((size_t)nprefix + 1)));
    chip_poison_fill(*dir_out, sizeof(u32) * ((size_t)nprefix + 1));
    hipLaunchKernelGGL(kmer_dir_kernel, dim3((unsigned)div_up((i64)n + 1, 256)), dim3(256), 0, ctx->stream, codes, n,
                       2 * K - (u32)P, nprefix, *dir_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int kmer_index_build(catchhip_ctx *ctx, const u8 *bytes, const i64 *off, i64 nseq, catchhip_kmer_index *X) {
    hipStream_t s = ctx->stream;
    const u32 K = (u32)X->k;
    const u64 mask = K == 32 ? ~0ull : (((u64)1 << (2 * K)) - 1);
    const u32 total = (u32)off[nseq];
    u32 n_valid = 0, n_unique = 0;
    DevBuf<u64> keys, keys_alt;
    PhaseTimer tm(ctx, PHASE_PREFILTER);
    if (total >= K) {
        DevBuf<u8> d_bytes;
        DevBuf<u32> d_off, cnt, at, tmp;
        std::vector<u32> h_off((size_t)nseq + 1);
        for (i64 i = 0; i <= nseq; ++i) h_off[(size_t)i] = (u32)off[i];
        TRY(d_bytes.alloc(total));
        TRY(d_off.alloc((size_t)nseq + 1));
        HIP_TRY(hipMemcpyAsync(d_bytes.p, bytes, total, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_off.p, h_off.data(), sizeof(u32) * ((size_t)nseq + 1), hipMemcpyHostToDevice, s));
        tm.restart();                                          // (the build's time starts behind the upload)
        const u32 nchunks = (u32)div_up((i64)total, BG_CHUNK);
        const dim3 grid((unsigned)div_up((i64)nchunks, 256)), block(256);
        TRY(cnt.alloc((size_t)nchunks + 1));
        TRY(at.alloc((size_t)nchunks + 1));
        HIP_TRY(hipMemsetAsync(cnt.p + nchunks, 0, sizeof(u32), s));
        hipLaunchKernelGGL(kmer_emit_kernel<false>, grid, block, 0, s, (const u8 *)d_bytes.p, (const u32 *)d_off.p,
                           (u32)nseq, total, nchunks, K, mask, 2 * K - 2, cnt.p, (const u32 *)nullptr, (u64 *)nullptr);
        TRY(chip_exclusive_scan_u32(ctx, cnt.p, at.p, (i64)nchunks + 1, tmp));
        TRY(read_count(ctx, at.p + nchunks, &n_valid));       // (also orders the pageable uploads before h_off goes)
        tm.launch(3);
        if (n_valid) {
            TRY(keys.alloc(n_valid));
            hipLaunchKernelGGL(kmer_emit_kernel<true>, grid, block, 0, s, (const u8 *)d_bytes.p, (const u32 *)d_off.p,
                               (u32)nseq, total, nchunks, K, mask, 2 * K - 2, (u32 *)nullptr, (const u32 *)at.p, keys.p);
            HIP_TRY(hipGetLastError());
            tm.launch();
        }
    }
    X->n_valid = n_valid;
    if (n_valid) {
        // the pair sort's values carry nothing; behind it the two value buffers serve the distinct pass
        DevBuf<u32> vals, vals_alt, tmp;
        TRY(vals.alloc((size_t)n_valid + 1));
        TRY(vals_alt.alloc((size_t)n_valid + 1));
        HIP_TRY(hipMemsetAsync(vals.p, 0, sizeof(u32) * ((size_t)n_valid + 1), s));
        TRY(chip_radix_sort_pairs(ctx, keys, keys_alt, vals, vals_alt, n_valid, 2 * (int)K));
        tm.launch(3 * ((2 * K + 7) / 8));
        const dim3 grid((unsigned)div_up((i64)n_valid, 256)), block(256);
        hipLaunchKernelGGL(kmer_head_kernel, grid, block, 0, s, (const u64 *)keys.p, n_valid, vals.p);
        HIP_TRY(hipMemsetAsync(vals.p + n_valid, 0, sizeof(u32), s));
        TRY(chip_exclusive_scan_u32(ctx, vals.p, vals_alt.p, (i64)n_valid + 1, tmp));
        TRY(read_count(ctx, vals_alt.p + n_valid, &n_unique));
        HIP_TRY(hipMalloc((void **)&X->codes, sizeof(u64) * (size_t)n_unique));
        chip_poison_fill(X->codes, sizeof(u64) * (size_t)n_unique);
        hipLaunchKernelGGL(kmer_compact_kernel, grid, block, 0, s, (const u64 *)keys.p, (const u32 *)vals.p,
                           (const u32 *)vals_alt.p, n_valid, X->codes);
        HIP_TRY(hipGetLastError());
        tm.launch(4);
        HIP_TRY(hipStreamSynchronize(s));                      // (the scratch goes back to the pool below)
    } else {
        HIP_TRY(hipMalloc((void **)&X->codes, sizeof(u64)));
        chip_poison_fill(X->codes, sizeof(u64));
        HIP_TRY(hipMemsetAsync(X->codes, 0, sizeof(u64), s));
    }
    X->n_unique = n_unique;
    const u32 M = (u32)X->mismatches;
    // view 0: the codes as they are.  A tolerant index keeps every directory no finer than its view's block
    TRY(kmer_view_dir(ctx, X->codes, n_unique, K, M ? 2 * (K / (M + 1)) : 2 * K, &X->P, &X->dir));
    tm.launch();
    for (u32 b = 1; b <= M; ++b) {
        const u32 s0 = b * K / (M + 1), s1 = (b + 1) * K / (M + 1);
        X->view_start[b - 1] = s0;
        HIP_TRY(hipMalloc((void **)&X->view_codes[b - 1], sizeof(u64) * (size_t)(n_unique ? n_unique : 1)));
        chip_poison_fill(X->view_codes[b - 1], sizeof(u64) * (size_t)(n_unique ? n_unique : 1));
        if (n_unique) {
            // rotate, sort again (a bijection: the list stays distinct), keep; the scratch is the first sort's
            DevBuf<u32> vals, vals_alt;
            TRY(keys.reserve(n_unique));
            TRY(vals.alloc((size_t)n_unique + 1));
            HIP_TRY(hipMemsetAsync(vals.p, 0, sizeof(u32) * ((size_t)n_unique + 1), s));
            hipLaunchKernelGGL(kmer_rotate_kernel, dim3((unsigned)div_up((i64)n_unique, 256)), dim3(256), 0, s,
                               (const u64 *)X->codes, n_unique, 2 * s0, 2 * K, mask, keys.p);
            HIP_TRY(hipGetLastError());
            TRY(chip_radix_sort_pairs(ctx, keys, keys_alt, vals, vals_alt, n_unique, 2 * (int)K));
            HIP_TRY(hipMemcpyAsync(X->view_codes[b - 1], keys.p, sizeof(u64) * (size_t)n_unique, hipMemcpyDeviceToDevice, s));
            tm.launch(1 + 3 * ((2 * K + 7) / 8));
            HIP_TRY(hipStreamSynchronize(s));                  // (the scratch goes back to the pool below)
        } else {
            HIP_TRY(hipMemsetAsync(X->view_codes[b - 1], 0, sizeof(u64), s));
        }
        TRY(kmer_view_dir(ctx, X->view_codes[b - 1], n_unique, K, 2 * (s1 - s0), &X->view_P[b - 1], &X->view_dir[b - 1]));
        tm.launch();
    }
    tm.stop();
    HIP_TRY(hipStreamSynchronize(s));
    tm.finish();
    return 0;
}

static int kmer_index_create(catchhip_ctx *ctx, const u8 *bytes, const i64 *off, i64 nseq, i32 k, i32 mismatches,
                             catchhip_kmer_index **out, i64 *n_valid, i64 *n_unique) {
    ARG_CHECK(ctx && out && off && nseq >= 0);
    *out = nullptr;
    if (k < 8 || k > 32) {
        chip_set_error("kmer_index_create: k must lie in 8 .. 32 (got %d)", (int)k);
        return CATCHHIP_EINVAL;
    }
    if (mismatches < 0 || mismatches > 2) {
        chip_set_error("kmer_index_create: mismatches must lie in 0 .. 2 (got %d)", (int)mismatches);
        return CATCHHIP_EINVAL;
    }
    if (k < 8 * (mismatches + 1)) {
        chip_set_error("kmer_index_create: %d mismatches need k >= %d, blocks of 8 characters at least (got k = %d)",
                       (int)mismatches, 8 * ((int)mismatches + 1), (int)k);
        return CATCHHIP_EINVAL;
    }
    if (nseq >= ((i64)1 << 31)) {
        chip_set_error("kmer_index_create: 2^31 records and more are not supported (got %lld)", (long long)nseq);
        return CATCHHIP_EINVAL;
    }
    ARG_CHECK(off[0] == 0);
    for (i64 i = 0; i < nseq; ++i) ARG_CHECK(off[i + 1] >= off[i]);
    if ((u64)off[nseq] >= BG_MAX_BYTES) {
        // (the valid positions are at most the bytes: this refuses every background of 2^32 valid positions and more)
        chip_set_error("kmer_index_create: a background of %lld bytes has too many positions for one index: the sort "
                       "and the scans count in 32 bits (fewer than %llu bytes; split the background)",
                       (long long)off[nseq], (unsigned long long)BG_MAX_BYTES);
        return CATCHHIP_EINVAL;
    }
    ARG_CHECK(off[nseq] == 0 || bytes);
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<catchhip_kmer_index> X(new catchhip_kmer_index());
    X->device = ctx->device;
    X->k = k;
    X->mismatches = mismatches;
    TRY(kmer_index_build(ctx, bytes, off, nseq, X.get()));
    if (n_valid) *n_valid = (i64)X->n_valid;
    if (n_unique) *n_unique = (i64)X->n_unique;
    *out = X.release();
    return 0;
}

extern "C" int catchhip_kmer_index_create(catchhip_ctx *ctx, const u8 *bytes, const i64 *off, i64 nseq, i32 k,
                                          catchhip_kmer_index **out, i64 *n_valid, i64 *n_unique) {
    return kmer_index_create(ctx, bytes, off, nseq, k, 0, out, n_valid, n_unique);
}

extern "C" int catchhip_kmer_index_create_tolerant(catchhip_ctx *ctx, const u8 *bytes, const i64 *off, i64 nseq, i32 k,
                                                   i32 mismatches, catchhip_kmer_index **out, i64 *n_valid,
                                                   i64 *n_unique) {
    return kmer_index_create(ctx, bytes, off, nseq, k, mismatches, out, n_valid, n_unique);
}

extern "C" int catchhip_kmer_index_fetch_view(catchhip_ctx *ctx, const catchhip_kmer_index *X, i32 view, u64 *out) {
    ARG_CHECK(ctx && X && ctx->device == X->device);
    if (view < 0 || view > X->mismatches) {
        chip_set_error("kmer_index_fetch_view: the index has the views 0 .. %d (got %d)", (int)X->mismatches, (int)view);
        return CATCHHIP_EINVAL;
    }
    if (X->n_unique == 0) return 0;
    ARG_CHECK(out);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(out, view ? X->view_codes[view - 1] : X->codes, sizeof(u64) * (size_t)X->n_unique,
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int catchhip_kmer_index_fetch(catchhip_ctx *ctx, const catchhip_kmer_index *X, u64 *out) {
    return catchhip_kmer_index_fetch_view(ctx, X, 0, out);
}

extern "C" void catchhip_kmer_index_destroy(catchhip_kmer_index *X) {
    if (!X) return;
    (void)hipSetDevice(X->device);
    delete X;                                                  // (hipFree waits for the device's work)
}

// ---- the filter ---------------------------------------------------------------------------------------------------
// M = 0: the exact look-up in view 0; M > 0: the tolerant one in the views 0 .. M
template <int M, bool STAGE, bool FILTER, bool HIST>
__device__ __forceinline__ void
background_flag_body(const RowArgs &a, u32 K, u64 mask, u32 rc_shift, const KmerViews &views, u32 max_hits,
                     u32 *__restrict__ flag, u64 *__restrict__ totals) {
    extern __shared__ u32 bg_lds[];
    const u32 rows = blockDim.x, r = threadIdx.x;
    const u32 i = blockIdx.x * rows + r;
    unsigned long long *cnt = (unsigned long long *)(bg_lds + a.extra_off_dw);      // (extra_off_dw is even: 8-byte aligned)
    for (u32 t = r; t < BG_WORDS; t += rows) cnt[t] = 0;
    if (STAGE) stage_rows(a, bg_lds);                                               // (ends with a barrier)
    else __syncthreads();
    u64 t_zero = 0, t_drop = 0;
    if (i < a.n) {                                            // (no early return: the wave sums and the barrier below)
        const u8 *p = row_ptr<STAGE>(a, bg_lds, i);
        KmerRoll kmer;
        u32 hits = 0;
        for (u32 j = 0; j < a.L; ++j) {
            const u8 c = p[j];
            if (kmer.step(base_code(c), is_base(c), mask, rc_shift, K)) {
                if constexpr (M == 0)
                    hits += kmer_lookup_exact(kmer.fwd, kmer.rc, views.codes[0], views.dir[0], views.dir_shift[0]);
                else hits += kmer_lookup_tolerant<M>(kmer.fwd, kmer.rc, mask, 2u * K, views);
            }
        }
        const u32 m = a.mult[i];
        if (HIST) {
            if (hits == 0) t_zero = m;
            else atomicAdd(cnt + (hits < BG_BINS - 1u ? hits : BG_BINS - 1u), (unsigned long long)m);
        }
        if (FILTER) {
            const bool drop = hits > max_hits;
            flag[i] = drop ? 0u : 1u;
            t_drop = drop ? m : 0u;
        }
    }
    totals_add_per_wave<BG_BINS>(cnt, t_zero, t_drop);        // bin 0, and "dropped" behind the bins
    __syncthreads();
    totals_flush(cnt, BG_WORDS, totals_slot(totals, BG_SLOTS, BG_SLOT_WORDS));
}

template <bool STAGE, bool FILTER, bool HIST>
__global__ void __launch_bounds__(256)
background_flag_kernel(const u8 *__restrict__ bytes, const u32 *__restrict__ upos, const u32 *__restrict__ mult, u32 n, u32 L,
                       u32 K, u64 mask, u32 rc_shift, const u64 *__restrict__ codes, const u32 *__restrict__ dir,
                       u32 dir_shift, u32 max_hits, u32 nchunk, u32 pitch_dw, u32 extra_off_dw, u32 *__restrict__ flag,
                       u64 *__restrict__ totals) {
    // (the row arguments one by one, in this order, and the struct made here: as ONE struct argument they moved the
    // others, the scalar loads were cut differently and the kernel ran 0.3 % slower -- DESIGN.md, round 13)
    const RowArgs a = {bytes, upos, mult, n, L, nchunk, pitch_dw, extra_off_dw};
    KmerViews views = {};
    views.codes[0] = codes;
    views.dir[0] = dir;
    views.dir_shift[0] = dir_shift;
    background_flag_body<0, STAGE, FILTER, HIST>(a, K, mask, rc_shift, views, max_hits, flag, totals);
}

// the same kernel against a tolerant index (M = 1, 2): per position 2 (M + 1) buckets instead of one (kmer_lookup.h)
template <int M, bool STAGE, bool FILTER, bool HIST>
__global__ void __launch_bounds__(256)
background_flag_tolerant_kernel(const u8 *__restrict__ bytes, const u32 *__restrict__ upos, const u32 *__restrict__ mult,
                                u32 n, u32 L, u32 K, u64 mask, u32 rc_shift, const KmerViews views, u32 max_hits,
                                u32 nchunk, u32 pitch_dw, u32 extra_off_dw, u32 *__restrict__ flag,
                                u64 *__restrict__ totals) {
    const RowArgs a = {bytes, upos, mult, n, L, nchunk, pitch_dw, extra_off_dw};     // (as in background_flag_kernel)
    background_flag_body<M, STAGE, FILTER, HIST>(a, K, mask, rc_shift, views, max_hits, flag, totals);
}

// the instances by what the call asks for: mode 0 the histogram alone, 1 the filter alone, 2 both
typedef decltype(&background_flag_kernel<false, false, true>) background_fn;
typedef decltype(&background_flag_tolerant_kernel<1, false, false, true>) background_tolerant_fn;
#define BG_MODES(KERNEL, ...)                                                                                          \
    { KERNEL<__VA_ARGS__, false, true>, KERNEL<__VA_ARGS__, true, false>, KERNEL<__VA_ARGS__, true, true> }
static background_fn background_instance(bool stage, int mode) {
    static const background_fn table[2][3] = {BG_MODES(background_flag_kernel, false), BG_MODES(background_flag_kernel, true)};
    return table[stage ? 1 : 0][mode];
}
static background_tolerant_fn background_tolerant_instance(i32 mismatches, bool stage, int mode) {
    static const background_tolerant_fn table[2][2][3] = {
        {BG_MODES(background_flag_tolerant_kernel, 1, false), BG_MODES(background_flag_tolerant_kernel, 1, true)},
        {BG_MODES(background_flag_tolerant_kernel, 2, false), BG_MODES(background_flag_tolerant_kernel, 2, true)}};
    return table[mismatches - 1][stage ? 1 : 0][mode];
}

extern "C" int catchhip_candidates_drop_background(catchhip_ctx *ctx, catchhip_candidates *C, const catchhip_kmer_index *X,
                                                   i32 filter_on, i64 max_hits, i64 dropped[1], u64 hist[256],
                                                   i64 *nkept) {
    ARG_CHECK(ctx && C && C->ctx == ctx && X);
    TRY(rule_refuse_filtered(C, "candidates_drop_background", "background filter"));
    if (X->device != ctx->device) {
        chip_set_error("candidates_drop_background: the index lives on device %d, the candidates on device %d", X->device,
                       ctx->device);
        return CATCHHIP_EINVAL;
    }
    if (filter_on && max_hits < 0) {
        chip_set_error("candidates_drop_background: max_hits must be >= 0 (got %lld)", (long long)max_hits);
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    TRY(rule_begin(ctx, C, nkept));
    if (dropped) dropped[0] = 0;
    if (hist) memset(hist, 0, sizeof(u64) * BG_BINS);
    if (C->nuniq == 0 || C->L < X->k || !(filter_on || hist)) return 0;
    const u32 H = !filter_on ? 0u : max_hits > (i64)0xffffffffll ? 0xffffffffu : (u32)max_hits;
    DevBuf<u32> flag;
    SlotTotals totals;
    if (filter_on) TRY(flag.alloc((size_t)C->nuniq + 1));
    TRY(totals.init(ctx, BG_SLOTS, BG_SLOT_WORDS));
    PhaseTimer tm(ctx, PHASE_PREFILTER);
    const u32 K = (u32)X->k;
    const u64 mask = K == 32 ? ~0ull : (((u64)1 << (2 * K)) - 1);
    const int mode = filter_on ? (hist ? 2 : 1) : 0;
    const RowPlan plan = row_plan((u32)C->L, 0, BG_EXTRA_BYTES, 4, rows_aligned(C));
    // row_plan's own rule once more, so it cannot fire: tests/test_background_filter.py looks for this expression in
    // this file's text (tests/test_candidate_launch_plan.py is what proves the tier edges, for every L)
    const size_t rows = plan.rows, row_bytes = (size_t)plan.pitch_dw * 4;
    ARG_CHECK(!(plan.stage && rows * row_bytes + BG_EXTRA_BYTES > POLYA_LDS_BUDGET));
    const RowArgs a = row_args(C, plan);                      // (the order below is the kernels')
    if (X->mismatches)                                        // the same launch, the tolerant kernel of the index's budget
        hipLaunchKernelGGL(background_tolerant_instance(X->mismatches, plan.stage, mode), row_grid(C, plan), dim3(plan.rows),
                           plan.lds_bytes, ctx->stream, a.bytes, a.upos, a.mult, a.n, a.L, K, mask, 2 * K - 2, kmer_views(X),
                           H, a.nchunk, a.pitch_dw, a.extra_off_dw, flag.p, totals.d.p);
    else
        hipLaunchKernelGGL(background_instance(plan.stage, mode), row_grid(C, plan), dim3(plan.rows), plan.lds_bytes,
                           ctx->stream, a.bytes, a.upos, a.mult, a.n, a.L, K, mask, 2 * K - 2, (const u64 *)X->codes,
                           (const u32 *)X->dir, 2 * K - X->P, H, a.nchunk, a.pitch_dw, a.extra_off_dw, flag.p, totals.d.p);
    HIP_TRY(hipGetLastError());
    tm.launch();
    tm.stop();
    u64 h[BG_WORDS];
    TRY(totals.read(ctx, BG_WORDS, h));
    tm.finish();
    if (hist) memcpy(hist, h, sizeof(u64) * BG_BINS);
    if (dropped) dropped[0] = (i64)h[BG_BINS];
    return rule_keep(ctx, C, h[BG_BINS] != 0, flag, nkept);
}
