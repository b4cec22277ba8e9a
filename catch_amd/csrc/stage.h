// What the candidate rule kernels share on the device (prefilter.hip, thermo.hip, background.hip, measure.hip; the
// totals also structure.hip): the rows of a workgroup in LDS, the per-byte steppers of a candidate's walk, and the
// padded copies of the totals.  Device code only; rule_host.h plans the launches that go with it.
#pragma once
#include "internal.h"
#include "wave.h"

// ---- rows ----------------------------------------------------------------------------------------------------------
// One thread per unique candidate.  A candidate's characters sit in the targets' byte array at upos[i] and the
// candidates of a workgroup overlap (stride < length), so the workgroup first copies its rows into LDS -- 16-byte loads
// from the 16-byte boundary below each row's start (<= 15 bytes before it), consecutive lanes on consecutive chunks of
// a row -- and the walk reads LDS.  The row pitch is an odd number of dwords: the lanes of a wave read the same column
// of 64 different rows, which an even pitch would put on a few banks.  Rows too long for 64 of them to fit the LDS
// budget are read from global memory (L is not bounded): STAGE = false.
struct RowArgs {
    const u8 *bytes;
    const u32 *upos, *mult;
    u32 n, L, nchunk, pitch_dw;
    // LDS: where what lies behind the staged rows begins (0 when they are not staged) -- the per-row extras, and
    // behind rows * (their dwords) the per-workgroup ones.  The Tm and background kernels, which have no per-row
    // extras, find their per-workgroup table and counters here; a family with both kinds passes the second offset
    // (RowPlan::tail_off_dw) as an argument of its own, as measure_rows_kernel does.
    u32 extra_off_dw;
};

// the rows of this workgroup (one per thread) into LDS, every thread of the workgroup calling; ends with a barrier
__device__ __forceinline__ void stage_rows(const RowArgs &a, u32 *lds) {
    const u32 rows = blockDim.x, base = blockIdx.x * rows;
    for (u32 t = threadIdx.x; t < rows * a.nchunk; t += rows) {
        const u32 row = t / a.nchunk, c = t - row * a.nchunk;
        if (base + row >= a.n) break;                     // (rows ascend with t)
        const u32 s = a.upos[base + row];
        const u32 at = (s & ~15u) + 16u * c;              // < s + L <= total: at most 15 bytes of the slack are read
        if (at >= s + a.L) continue;
        const uint4 v = *(const uint4 *)(a.bytes + at);
        u32 *d = lds + row * a.pitch_dw + 4u * c;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
}

// candidate i's characters as this thread walks them: its staged row, or the byte array
template <bool STAGE> __device__ __forceinline__ const u8 *row_ptr(const RowArgs &a, const u32 *lds, u32 i) {
    const u32 s = a.upos[i];
    return STAGE ? (const u8 *)(lds + threadIdx.x * a.pitch_dw) + (s & 15u) : a.bytes + s;
}

__device__ __forceinline__ bool is_base(u8 c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
// 'A' 0, 'C' 1, 'T' 2, 'G' 3 (a 32-bit argument: on a byte the compiler shifts in 16 bits and masks, two instructions for one)
__device__ __forceinline__ u32 base_code(u32 c) { return (c >> 1) & 3u; }

// ---- per-byte steppers: the state of one candidate's walk, in registers ----------------------------------------------
// The triplet counters of the low-complexity window (composition_flag_kernel in prefilter.hip and measure_rows_kernel
// each write the window's step out; prefilter.hip says why).  The counters c_t of the 64 triplet codes are indexed by
// data, so they live in LDS, one byte each (a window of <= 256 bytes holds <= 254 triplets): TRIPLET_COUNTER_BYTES per
// thread behind the staged rows.  Layout: dword g * rows + r holds the counters of codes 4g .. 4g + 3 of thread r -- a
// lane's pitch is ONE dword and a code group's pitch is `rows` dwords (a multiple of 32), so whatever codes the lanes
// of a wave touch, lane l is on bank l mod 32: the 32 lanes that a byte access serves per cycle never share a bank.  A
// thread touches its own counters only (no barrier).
#define TRIPLET_COUNTER_BYTES 64u

// Nearest-neighbour melting temperature.  |h| | |e| << 16 of the dinucleotide (first, second), index 4 * first +
// second in base_code()'s numbering: SantaLucia 1998, h in 100 cal/mol, e in 0.1 cal/(K mol).  The table is indexed by
// data, so the kernels copy it into LDS: 16 consecutive dwords are 16 different banks, and lanes on one dword are
// served by a broadcast, so whatever dinucleotides the lanes of a wave hold the look-up has no bank conflict.  Only
// the table's entries are packed: the two sums are 64-bit registers each (|E| passes 65,535 at 300 bases, |H| at
// 1,000, and L is not bounded); the initiation terms and the signs are applied after the walk.  Then
//     E' = 100 E + q,   T = H < 0 ? 10^7 (-H) / (-E') : 0,   tm_c = T - offset_c
// with ONE unsigned 64-bit division per candidate; q <= -8200 keeps E' negative wherever H < 0 (the host checks it).
#define TM_TABLE_DW 16u
#define TM_NN(h, e) ((u32)(h) | ((u32)(e) << 16))
// (static: every file that includes this header gets its own 64 bytes of constant memory, read or not -- by design,
// the library is not built with relocatable device code, so a table shared between files would need a host copy)
__attribute__((unused)) static __constant__ u32 tm_nn_table[TM_TABLE_DW] = {
    TM_NN(79, 222), TM_NN(84, 224), TM_NN(72, 204), TM_NN(78, 210),       // AA AC AT AG
    TM_NN(85, 227), TM_NN(80, 199), TM_NN(78, 210), TM_NN(106, 272),      // CA CC CT CG
    TM_NN(72, 213), TM_NN(82, 222), TM_NN(79, 222), TM_NN(85, 227),       // TA TC TT TG
    TM_NN(82, 222), TM_NN(98, 244), TM_NN(84, 224), TM_NN(80, 199)};      // GA GC GT GG

struct TmSums {
    u64 sh = 0, se = 0;                                       // -sum of h, -sum of e over the dinucleotides
    u32 pc = 0;
    bool pb = false;
    // the table into LDS, the first TM_TABLE_DW threads of the workgroup; a barrier must follow before step()
    static __device__ __forceinline__ void load_table(u32 *tbl) {
        if (threadIdx.x < TM_TABLE_DW) tbl[threadIdx.x] = tm_nn_table[threadIdx.x];
    }
    __device__ __forceinline__ void step(const u32 *tbl, u32 code, bool b) {
        const u32 e = (b && pb) ? tbl[(pc << 2) | code] : 0u;
        sh += e & 0xffffu;
        se += e >> 16;
        pc = code;
        pb = b;
    }
    __device__ __forceinline__ i64 tm_c(u8 first, u8 last, i64 q, i64 offset_c) const {
        const bool g0 = first == 'G' || first == 'C', g1 = last == 'G' || last == 'C';
        const i64 H = (g0 ? 1 : 23) + (g1 ? 1 : 23) - (i64)sh;
        const i64 E = (g0 ? -28 : 41) + (g1 ? -28 : 41) - (i64)se;
        const i64 E1 = 100 * E + q;                           // < 0 wherever H < 0
        const i64 T = H < 0 ? (i64)((10000000ull * (u64)(-H)) / (u64)(-E1)) : 0;
        return T - offset_c;
    }
};

// The k-mer that ends at this byte, rolled (background.hip's head defines the code): fwd and the code of its reverse
// complement rc, and the run of bases that ends here -- from run >= K on the two hold exactly the last K characters.
struct KmerRoll {
    u64 fwd = 0, rc = 0;
    u32 run = 0;
    // true: fwd and rc are a valid k-mer's (the caller looks them up, kmer_lookup.h)
    __device__ __forceinline__ bool step(u64 code, bool b, u64 mask, u32 rc_shift, u32 K) {
        fwd = ((fwd << 2) | code) & mask;
        rc = (rc >> 2) | ((code ^ 2ull) << rc_shift);
        run = b ? run + 1u : 0u;
        return run >= K;
    }
};

// ---- totals ---------------------------------------------------------------------------------------------------------
// A family's totals (with multiplicity) live in `slots` padded copies in global memory, slot_words 64-bit words apart
// (whole 128-byte lines), and the host adds the copies up (rule_host.h: SlotTotals).  The copy is chosen by the
// workgroup's number.  With one copy, the 140,000 waves of 8.9 M candidates queued on a single line and the atomics
// took longer than the walk.  Two ways in: per wave, for a few totals most threads add to; per workgroup through
// counters in LDS, for histograms.
__device__ __forceinline__ unsigned long long *totals_slot(u64 *totals, u32 slots, u32 slot_words) {
    return (unsigned long long *)totals + (size_t)(blockIdx.x & (slots - 1u)) * slot_words;
}
// values summed over the wave (wave_sum_n: every lane calls), then one atomic per wave and non-zero value: value k
// goes to t[k * STRIDE] (global memory, or counters in LDS that totals_flush takes on)
template <u32 STRIDE = 1, typename... T> __device__ __forceinline__ void totals_add_per_wave(unsigned long long *t, T... v) {
    wave_sum_n(v...);
    if ((threadIdx.x & 63u) == 0) {
        u32 k = 0;
        ((v ? (void)atomicAdd(t + STRIDE * k++, (unsigned long long)v) : (void)k++), ...);
    }
}
// after a barrier: thread t adds LDS counter t, if it is not zero, to word at(t) of the workgroup's copy -- a wave's
// adds are neighbouring u64s of a few 128-byte lines
template <typename F>
__device__ __forceinline__ void totals_flush(const unsigned long long *cnt, u32 nwords, unsigned long long *slot, F at) {
    for (u32 t = threadIdx.x; t < nwords; t += blockDim.x) {
        const unsigned long long v = cnt[t];
        if (v) atomicAdd(slot + at(t), v);
    }
}
__device__ __forceinline__ void totals_flush(const unsigned long long *cnt, u32 nwords, unsigned long long *slot) {
    totals_flush(cnt, nwords, slot, [](u32 t) { return t; });
}
