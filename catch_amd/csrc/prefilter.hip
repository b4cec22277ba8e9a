// Filters that are a function of the candidate alone, on the device's candidate list -- they run before the
// near-duplicate filter and the set cover, where the reference runs them before the duplicate filter.
//
// PolyAFilter (catch/filter/polya_filter.py:43-71): a candidate is dropped iff
//   * it holds an exact run of >= min_exact 'A' or of >= min_exact 'T' (the reference's gate before its slow
//     call; it changes answers, so it is part of the rule; min_exact == 0 lets everything through), and
//   * for c = 'A' or c = 'T' its longest common substring with c * L under `mismatches` mismatches
//     (Probe.longest_common_substring_length, an O(L^2) k_lcf per candidate) is >= length.
// The second condition asks for a window of >= length characters of which at most `mismatches` differ from c.
// Every such window contains one of exactly `length` characters with no more mismatches, so "the longest window
// is >= length" is "some window of `length` characters has <= mismatches mismatches": two pointers `length`
// apart, one pass, the same two characters read for 'A' and for 'T'.  Any character but c is a mismatch ('N' too).
//
// polya_flag_kernel: one thread per unique candidate, O(L).  A candidate's characters sit in the targets' byte
// array at upos[i] and the candidates of a workgroup overlap (stride < length), so the workgroup first copies its
// rows into LDS -- 16-byte loads from the 16-byte boundary below each row's start, consecutive lanes on
// consecutive chunks of a row -- and both pointers of the walk read LDS.  The row pitch is an odd number of
// dwords: the lanes of a wave read the same column of 64 different rows, which an even pitch would put on a
// few banks.  Rows too long for 64 of them to fit the LDS budget are read from global memory (L is not bounded).
#include "internal.h"

#define POLYA_LDS_BUDGET 65536u

template <bool STAGE>
__global__ void __launch_bounds__(256)
polya_flag_kernel(const u8 *__restrict__ bytes, const u32 *__restrict__ upos, u32 n, u32 L, u32 length, u32 k,
                  u32 min_exact, u32 nchunk, u32 pitch_dw, u32 *__restrict__ flag) {
    extern __shared__ u32 polya_lds[];
    const u32 rows = blockDim.x, r = threadIdx.x;
    const u32 base = blockIdx.x * rows;
    if (STAGE) {
        for (u32 t = r; t < rows * nchunk; t += rows) {
            const u32 row = t / nchunk, c = t - row * nchunk;
            if (base + row >= n) break;                       // (rows ascend with t)
            const u32 s = upos[base + row];
            const u32 a = (s & ~15u) + 16u * c;               // < s + L <= total: at most 15 bytes of the slack are read
            if (a >= s + L) continue;
            const uint4 v = *(const uint4 *)(bytes + a);
            u32 *d = polya_lds + row * pitch_dw + 4u * c;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        __syncthreads();
    }
    const u32 i = base + r;
    if (i >= n) return;
    const u32 s = upos[i];
    const u8 *p = STAGE ? (const u8 *)(polya_lds + r * pitch_dw) + (s & 15u) : bytes + s;
    u32 mm_a = 0, mm_t = 0, run_a = 0, run_t = 0, best_run = 0;
    bool hit = false;
    for (u32 j = 0; j < L; ++j) {
        const u8 c = p[j];
        const bool a = c == 'A', t = c == 'T';
        run_a = a ? run_a + 1 : 0;
        run_t = t ? run_t + 1 : 0;
        best_run = max(best_run, max(run_a, run_t));
        mm_a += a ? 0u : 1u;
        mm_t += t ? 0u : 1u;
        if (j >= length) {
            const u8 o = p[j - length];
            mm_a -= o == 'A' ? 0u : 1u;
            mm_t -= o == 'T' ? 0u : 1u;
        }
        if (j + 1 >= length) hit |= mm_a <= k || mm_t <= k;
    }
    flag[i] = (hit && best_run >= min_exact) ? 0u : 1u;       // (min_exact == 0: every candidate passes the gate)
}

extern "C" int catchhip_candidates_drop_polya(catchhip_ctx *ctx, catchhip_candidates *C, i32 length, i32 mismatches,
                                              i32 min_exact, i64 *nkept) {
    ARG_CHECK(ctx && C && C->ctx == ctx);
    if (C->filtered) {
        chip_set_error("candidates_drop_polya: a near-duplicate filter was already applied (the poly(A) filter comes first)");
        return CATCHHIP_EINVAL;
    }
    if (length < 1 || mismatches < 0 || min_exact < 0) {
        chip_set_error("candidates_drop_polya: length must be >= 1, mismatches and min_exact >= 0 (got %d, %d, %d)",
                       (int)length, (int)mismatches, (int)min_exact);
        return CATCHHIP_EINVAL;
    }
    PoolScope pool_scope(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    if (nkept) *nkept = C->nuniq;
    if (C->nuniq == 0 || length > C->L) return 0;             // a stretch longer than the candidates: nothing to drop
    const u32 n = (u32)C->nuniq, L = (u32)C->L;
    DevBuf<u32> flag;
    TRY(flag.alloc((size_t)n + 1));
    // a row in LDS: from the 16-byte boundary below its start (<= 15 bytes before it) to its end
    const u32 nchunk = (L + 15u + 15u) / 16u, pitch_dw = 4u * nchunk + 1u;
    u32 rows = 256;
    while (rows > 64 && (size_t)rows * pitch_dw * 4 > POLYA_LDS_BUDGET) rows >>= 1;
    const bool stage = (size_t)rows * pitch_dw * 4 <= POLYA_LDS_BUDGET && ((uintptr_t)C->T->bytes.p & 15u) == 0;
    if (stage)
        hipLaunchKernelGGL(polya_flag_kernel<true>, dim3((unsigned)div_up((i64)n, rows)), dim3(rows),
                           (size_t)rows * pitch_dw * 4, ctx->stream, (const u8 *)C->T->bytes.p, (const u32 *)C->upos.p, n,
                           L, (u32)length, (u32)mismatches, (u32)min_exact, nchunk, pitch_dw, flag.p);
    else
        hipLaunchKernelGGL(polya_flag_kernel<false>, dim3((unsigned)div_up((i64)n, 256)), dim3(256), 0, ctx->stream,
                           (const u8 *)C->T->bytes.p, (const u32 *)C->upos.p, n, L, (u32)length, (u32)mismatches,
                           (u32)min_exact, nchunk, pitch_dw, flag.p);
    HIP_TRY(hipGetLastError());
    return chip_candidates_keep_flagged(ctx, C, flag, nkept);
}

// the multiplicities the filter must carry along (tests compare them; the near-duplicate filters read them on the device)
extern "C" int catchhip_candidates_multiplicities(catchhip_ctx *ctx, const catchhip_candidates *C, u32 *mult) {
    ARG_CHECK(ctx && C && C->ctx == ctx);
    if (C->filtered) {
        chip_set_error("candidates_multiplicities: not kept once a near-duplicate filter was applied");
        return CATCHHIP_EINVAL;
    }
    if (C->nuniq == 0) return 0;
    ARG_CHECK(mult);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(mult, C->mult.p, sizeof(u32) * (size_t)C->nuniq, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}
