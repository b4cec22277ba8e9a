// Row staging of the candidate pre-filters' flag kernels (prefilter.hip, thermo.hip): one thread per unique candidate,
// the rows of a workgroup copied into LDS first (prefilter.hip's head says why and how).  Device code only.
#pragma once
#include "internal.h"

#define POLYA_LDS_BUDGET 65536u

// the rows of this workgroup (one per thread) into LDS, every thread of the workgroup calling; ends with a barrier
__device__ __forceinline__ void stage_rows(const u8 *__restrict__ bytes, const u32 *__restrict__ upos, u32 n, u32 L,
                                           u32 nchunk, u32 pitch_dw, u32 *lds) {
    const u32 rows = blockDim.x, base = blockIdx.x * rows;
    for (u32 t = threadIdx.x; t < rows * nchunk; t += rows) {
        const u32 row = t / nchunk, c = t - row * nchunk;
        if (base + row >= n) break;                       // (rows ascend with t)
        const u32 s = upos[base + row];
        const u32 a = (s & ~15u) + 16u * c;               // < s + L <= total: at most 15 bytes of the slack are read
        if (a >= s + L) continue;
        const uint4 v = *(const uint4 *)(bytes + a);
        u32 *d = lds + row * pitch_dw + 4u * c;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
}

__device__ __forceinline__ bool is_base(u8 c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
