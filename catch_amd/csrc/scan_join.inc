// K1d: key-grouped join (included by scan.hip) -- the seed scan for pigeonhole tables since round 4.
//
// What the reference computes (catch/probe.py:1008-1119): for every target position i whose k-mer is a key of the
// anchor map, and every entry (probe, anchor) listed under that key, the cover function of the probe aligned at
// i - anchor; under the K1c conditions (SURVEY.md App. A.8) that is "Hamming(probe, window) <= m, the seeding anchor
// exact, reported from the lowest exact anchor".
//
// The seed-list scan (seed_lookup + seed_verify4, rounds 1-3) expanded the (position, entry) pairs into a work list
// ordered by position: 2.3e9 table matches -> 0.94e9 twelve-byte seeds per S4 step, every one of which gathered a
// 64-byte probe image at random (rocprofv3 PMC: 267 GB of L2-miss traffic per step for look-up + verify).  But the
// pairs are not a list, they are a union of BICLIQUES: all W positions that hold one k-mer pair with all Q entries
// listed under it (S4: W ~ 150 strains of a clade x Q ~ 120 of their probes at every anchor position).  So:
//   1. kj_hitpos:  every target position looks its k-mer up and files (slot, position, sequence) -- only the hit
//      positions, 1 in 25 (S4: 24 M records instead of 2.3e9 matches), in position order (per-workgroup staging +
//      a scan of the workgroup counts; the order is what makes every later list sorted without sorting it);
//   2. a stable radix sort of those records by table slot (the 25-bit slot number: 4 passes over 24 M records);
//   3. kj_verify: a wavefront takes a run of equal slots: its lanes hold one window each IN REGISTERS, pre-shifted
//      for every anchor of the table (<= KJ_AMAX x NW x 3 words), and the run's entries go by one after the other:
//      entry id and probe image arrive through the SCALAR cache (wave-uniform addresses), the Hamming test is
//      3 xor + or3 + bcnt per 32 bases, nothing is gathered per pair.  Windows are read once per run (24 M x 80 B),
//      probe images once per run (12 M x 64 B);
//   4. two passes of (3): the first counts the hits per entry, a scan turns the counts into the offsets of the row
//      build's bucket-grouped array (a bucket = the entries of a probe side by side), the second writes every hit
//      record at its final place, per entry in position order.  There is no hit list, no rank atomic and no
//      bucket scatter (14.6 ms per S4 step in round 3): the records are written once, densely.
// Runs of W <= 4 windows (a strain's private k-mer: millions of them, a pair or two each) are handled one per LANE;
// a run whose W x Q exceeds KJ_GIANT_PAIRS (low-complexity k-mers) is cut by entries into tasks for a second launch.
// Memory: 12 B per hit position + 4 B per anchor instead of 32 B per seed (S4's largest group: 38 GB -> 0.4 GB).

#define KJ_HT 512
#define KJ_PPT 4
#define KJ_TILE (KJ_HT * KJ_PPT)
#define KJ_AMAX 5                      // anchors of a probe in the table (m + 1 <= 5)
#define KJ_LANES_W 48u                 // runs of fewer windows ...
#define KJ_LANES_PAIRS 4096u           // ... and at most this many pairs get a lane per window (kj_lanes)
#define KJ_GIANT_PAIRS (1u << 15)      // pairs of one run a single wavefront takes; beyond: tasks of fewer entries
#define KJ_PRESENCE_BITS 3             // bits of its presence word a key sets and kj_hitpos tests (seed_presence)

__device__ __forceinline__ u32 seed_find_slot(const SeedTable &t, unsigned long long key, uint2 *range) {
    if (t.present) {
        u32 pw;
        const u32 pm = seed_presence(t, key, &pw);
        if ((t.present[pw] & pm) != pm) return SEED_SLOT_NONE;
    }
    u32 sl_i = seed_hash(key) & t.mask;
    for (;;) {
        const uint4 sl = t.slot[sl_i];
        const unsigned long long ks = ((unsigned long long)sl.y << 32) | sl.x;
        if (ks == key) { *range = make_uint2(sl.z, sl.w); return sl_i; }
        if (ks == SEED_EMPTY) return SEED_SLOT_NONE;
        sl_i = (sl_i + 1) & t.mask;
    }
}

// 1. hit positions of a tile, densely at the front of the tile's staging region, in position order
__global__ void __launch_bounds__(KJ_HT)
kj_hitpos_kernel(const u32 *__restrict__ tplanes, i64 nwords, u32 total, const u32 *__restrict__ seq_off, u32 nseq,
                 int k, int kb, SeedTable t, unsigned long long *__restrict__ stage_key, u32 *__restrict__ stage_sq,
                 u32 *__restrict__ wg_cnt) {
    __shared__ u32 s_part[KJ_HT / 64];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 tile0 = blockIdx.x * KJ_TILE;
    const u32 sq0 = find_segment(seq_off, nseq, min(tile0, total - 1));
    u32 slot[KJ_PPT], sqs[KJ_PPT], mine = 0;
    // Round 6: the thread's KJ_PPT positions in three batches -- keys and presence bits of all of them, then the first table
    // slot of those that passed, then the rest -- instead of one position after the other (each a chain presence bit ->
    // slot -> next slot: a wavefront of 256 positions holds ~10 hit positions and waited for up to four such chains in a row)
    unsigned long long key[KJ_PPT];
    bool cand[KJ_PPT];
    u32 at[KJ_PPT];
#pragma unroll
    for (int j = 0; j < KJ_PPT; ++j) {
        const u32 i = tile0 + tid * KJ_PPT + j;
        slot[j] = SEED_SLOT_NONE; sqs[j] = 0;
        cand[j] = i < total && i + (u32)k <= total;
        key[j] = cand[j] ? plane_key(tplanes, tplanes + nwords, i, kb) : 0ull;
        at[j] = seed_hash(key[j]) & t.mask;
    }
    if (t.present) {
        u32 pw[KJ_PPT], pm[KJ_PPT];
#pragma unroll
        for (int j = 0; j < KJ_PPT; ++j) { u32 w; pm[j] = seed_presence(t, key[j], &w); pw[j] = cand[j] ? t.present[w] : 0u; }
#pragma unroll
        for (int j = 0; j < KJ_PPT; ++j) cand[j] = cand[j] && (pw[j] & pm[j]) == pm[j];
    }
    uint4 first[KJ_PPT];
#pragma unroll
    for (int j = 0; j < KJ_PPT; ++j) first[j] = cand[j] ? t.slot[at[j]] : make_uint4(0xffffffffu, 0xffffffffu, 0u, 0u);
#pragma unroll
    for (int j = 0; j < KJ_PPT; ++j) {
        if (!cand[j]) continue;
        const u32 i = tile0 + tid * KJ_PPT + j;
        uint4 sl = first[j];
        u32 sl_i = at[j], f = SEED_SLOT_NONE;
        uint2 r = make_uint2(0, 0);
        for (;;) {
            const unsigned long long ks = ((unsigned long long)sl.y << 32) | sl.x;
            if (ks == key[j]) { r = make_uint2(sl.z, sl.w); f = sl_i; break; }
            if (ks == SEED_EMPTY) break;
            sl_i = (sl_i + 1) & t.mask;
            sl = t.slot[sl_i];
        }
        if (f != SEED_SLOT_NONE && r.y) {
            u32 sq = sq0;
            while (sq + 1 < nseq && seq_off[sq + 1] <= i) ++sq;
            if (i + (u32)k <= seq_off[sq + 1]) { slot[j] = f; sqs[j] = sq; ++mine; }   // the k-mer lies inside one sequence
        }
    }
    u32 wtotal;
    const u32 ex = wave_excl_scan(mine, &wtotal);
    if (lane == 0) s_part[wave] = wtotal;
    __syncthreads();
    u32 woff = 0, tot = 0;
    for (int w = 0; w < KJ_HT / 64; ++w) { if (w < (int)wave) woff += s_part[w]; tot += s_part[w]; }
    u32 o = tile0 + woff + ex;
#pragma unroll
    for (int j = 0; j < KJ_PPT; ++j)
        if (slot[j] != SEED_SLOT_NONE) {
            stage_key[o] = ((unsigned long long)slot[j] << 32) | (tile0 + tid * KJ_PPT + j);
            stage_sq[o] = sqs[j];
            ++o;
        }
    if (tid == 0) {
        wg_cnt[blockIdx.x] = tot;
        if (blockIdx.x == 0) wg_cnt[gridDim.x] = 0;   // (the scan's extra element: its prefix is the total)
    }
}

// the tiles' records, one after the other
__global__ void __launch_bounds__(64)
kj_compact_kernel(const unsigned long long *__restrict__ stage_key, const u32 *__restrict__ stage_sq,
                  const u32 *__restrict__ wg_off, unsigned long long *__restrict__ hkey, u32 *__restrict__ hsq) {
    const u32 b = blockIdx.x, o0 = wg_off[b], n = wg_off[b + 1] - o0, s0 = b * KJ_TILE;
    for (u32 d = threadIdx.x; d < n; d += 64) { hkey[o0 + d] = stage_key[s0 + d]; hsq[o0 + d] = stage_sq[s0 + d]; }
}

struct JoinArgs {
    const uint4 *tq; const u32 *seq_off; const uint4 *pplanes;
    int nanch, ntab, L, k, mm; u32 tailmask;
    unsigned long long div_magic;                 // ceil(2^34 / nanch)
    const unsigned long long *hkey; const u32 *hsq; u32 nhit;
    const uint4 *slot; const u32 *ents;
    u32 *ecnt;              // counting pass: hits per entry
    const u32 *ebase;       // writing pass: the entry's first record of S
    uint4 *S;               // {start, end, segment, bucket} (extended + clipped), grouped by bucket
    const u32 *bucket_of; const i32 *seq_genome; u32 ext;
    const i32 *probe_group; const i32 *seq_group;
    uint4 *giant; u32 *giant_n; u32 giant_cap;   // tasks {first hit, windows, first entry, entries}
    // hit masks: the counting pass keeps, per 64-entry block and 64-window chunk of a wave-wide run, one 64-bit
    // ballot per entry (which windows it hit); the writing pass replays them instead of testing every pair again.
    // mbase[first hit of the run] / gmbase[task] = where the run's masks start (KJ_NOMASK: the store was full,
    // the writing pass then verifies that run again); mcursor[64]: words handed out of each of the store's 64 parts
    // (one cursor would be one address: 10^6 runs x ~10 ns; S4i's count pass spent 9 of 16 ms there).
    unsigned long long *masks; u32 *mbase, *gmbase; unsigned long long *mcursor; u32 mask_cap;
    unsigned long long *pairs;                    // [0..64): pairs verified, [64..128): lane slots of the wave-wide runs (sharded counters)
};

template <int NW> struct KjWin { u32 x[NW], y[NW], z[NW]; };

// the NW words of the window that starts at base o, per plane
template <int NW>
__device__ __forceinline__ void kj_load_window(const uint4 *__restrict__ tq, u32 o, KjWin<NW> &w) {
    const u32 sh = o & 31u;
    const uint4 *tp = tq + (o >> 5);
    uint4 cur = tp[0];
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const uint4 nx = tp[j + 1];          // (the image has slack words beyond the last base)
        w.x[j] = __builtin_amdgcn_alignbit(nx.x, cur.x, sh);
        w.y[j] = __builtin_amdgcn_alignbit(nx.y, cur.y, sh);
        w.z[j] = __builtin_amdgcn_alignbit(nx.z, cur.z, sh);
        cur = nx;
    }
}

// <= mm mismatches, the seeding anchor a exact on all planes, every lower anchor broken (the pair is reported
// from its lowest exact anchor: catch/probe.py:1062-1119 finds it once per anchor, the merge keeps one).
// Branch-free: with a and k wave-uniform the word masks are scalars, a test is one v_and_or per word.
template <int NW>
__device__ __forceinline__ bool kj_accept(const u32 (&mw)[NW], u32 a, int k, int mm) {
    u32 cnt = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) cnt += __popc(mw[j]);
    u32 own = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) own |= mw[j] & word_range_mask(j, (int)a * k, k);
    bool ok = (cnt <= (u32)mm) & (own == 0u);
#pragma unroll
    for (u32 b = 0; b + 1 < KJ_AMAX; ++b) {
        u32 low = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) low |= mw[j] & word_range_mask(j, (int)b * k, k);
        ok = ok & ((b >= a) | (low != 0u));
    }
    return ok;
}

__device__ __forceinline__ uint4 kj_record(const JoinArgs &A, u32 p, u32 o, u32 sq, u32 lo, u32 hi) {
    const u32 ge = o + (u32)A.L;
    const u32 es = (o - lo > A.ext) ? o - A.ext : lo;
    const u32 ee = (hi - ge > A.ext) ? ge + A.ext : hi;
    return make_uint4(es, ee, A.seq_genome ? (u32)A.seq_genome[sq] : sq, A.bucket_of ? A.bucket_of[p] : p);
}

// One run of equal slots, the whole wavefront: windows [i0, i0 + W) of the sorted hit list against the entries
// ents[efirst .. efirst + nq).  All arguments are wave-uniform.  The entries go through LDS 64 at a time (KjLds, one
// per wavefront): every lane fetches one entry's probe image and bucket, and the block is laid out SORTED BY ANCHOR,
// so that the loop over a segment has a fixed anchor -- the window registers and the anchor masks it uses are
// static -- and reads its probe words as LDS broadcasts.  (First version: entry id and image through scalar loads
// inside the loop -- two dependent memory round trips per entry, ~1 us each: 38 + 49 ms per S4 step for the two
// passes, and a 4 ms tail behind every run of 4,000 entries.)
#define KJ_EB 64
#define KJ_NOMASK 0xffffffffu
template <int NW> struct KjLds {
    uint4 img[KJ_EB * NW];
    u32 b[KJ_EB];          // bucket of the entry's probe
    u32 eb[KJ_EB];         // counting pass: entry id; writing pass: the entry's first record
    i32 grp[KJ_EB];        // group of the probe (union instances)
};
#define KJ_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// The writing pass of a run whose hit masks were kept: no windows, no probe images, no bit work -- per 64-entry
// block only bucket and offset of the entries are staged, per chunk the lanes' positions, and the masks say who
// writes (the counting pass costs ~45 lane-ops per pair, this ~10 per (chunk, entry)).
template <int NW>
__device__ __forceinline__ void kj_replay(const JoinArgs &A, KjLds<NW> &sm, u32 i0, u32 W, u32 efirst, u32 nq, u32 mb,
                                          u32 lane) {
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    const u32 nanch = (u32)A.nanch, k = (u32)A.k, L = (u32)A.L;
    const u32 nchunks = (W + 63u) >> 6;
    for (u32 qb = 0; qb < nq; qb += KJ_EB) {
        const u32 nqb = min((u32)KJ_EB, nq - qb);
        u32 cnt_reg = 0;
        u32 segend[KJ_AMAX];
        {
            KJ_WAVE_SYNC();
            const bool valid = lane < nqb;
            const u32 e = valid ? A.ents[efirst + qb + lane] : 0u;
            const u32 p = e / nanch, a = e - p * nanch;
            u32 posn = 0, run = 0;
#pragma unroll
            for (int aa = 0; aa < KJ_AMAX; ++aa) {
                const unsigned long long m = __ballot(valid && a == (u32)aa);
                if (a == (u32)aa) posn = run + (u32)__popcll(m & lt);
                run += (u32)__popcll(m);
                segend[aa] = run;
            }
            if (valid) { sm.b[posn] = A.bucket_of ? A.bucket_of[p] : p; sm.eb[posn] = A.ebase[e]; }
            KJ_WAVE_SYNC();
        }
        for (u32 c = 0; c < nchunks; ++c) {
            const unsigned long long mine = A.masks[(size_t)mb + ((size_t)(qb >> 6) * nchunks + c) * 64u + lane];   // entry `lane` of the block
            if (!__ballot(mine != 0ull)) continue;
            const u32 mlo = (u32)mine, mhi = (u32)(mine >> 32);
            const u32 c0 = c << 6;
            const bool inw = c0 + lane < W;
            u32 pos = 0, sq = 0, lo = 0, hi = 0, seg = 0;
            if (inw) {
                pos = (u32)A.hkey[i0 + c0 + lane];
                sq = A.hsq[i0 + c0 + lane];
                lo = A.seq_off[sq]; hi = A.seq_off[sq + 1];
                seg = A.seq_genome ? (u32)A.seq_genome[sq] : sq;
            }
            u32 seg_lo = 0;
#pragma unroll
            for (int aa = 0; aa < KJ_AMAX; ++aa) {
                if (aa >= A.ntab) break;
                const u32 seg_hi = segend[aa];
                const u32 o = pos - (u32)aa * k, ge = o + L;
                const u32 es = (o - lo > A.ext) ? o - A.ext : lo;
                const u32 ee = (hi - ge > A.ext) ? ge + A.ext : hi;
                for (u32 j = seg_lo; j < seg_hi; ++j) {
                    const unsigned long long hb = ((unsigned long long)(u32)__builtin_amdgcn_readlane((int)mhi, (int)j) << 32) |
                                                  (unsigned long long)(u32)__builtin_amdgcn_readlane((int)mlo, (int)j);
                    if (!hb) continue;
                    const u32 base = (u32)__builtin_amdgcn_readlane((int)cnt_reg, (int)j);
                    if ((hb >> lane) & 1ull) A.S[sm.eb[j] + base + (u32)__popcll(hb & lt)] = make_uint4(es, ee, seg, sm.b[j]);
                    if (lane == j) cnt_reg = base + (u32)__popcll(hb);
                }
                seg_lo = seg_hi;
            }
        }
    }
}

// mb: where this run's hit masks go (counting pass; KJ_NOMASK: nowhere)
template <int NW, bool WRITE>
__device__ __forceinline__ void kj_big(const JoinArgs &A, KjLds<NW> &sm, u32 i0, u32 W, u32 efirst, u32 nq, u32 mb, u32 lane) {
    if (WRITE && mb != KJ_NOMASK) { kj_replay<NW>(A, sm, i0, W, efirst, nq, mb, lane); return; }
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    const u32 nanch = (u32)A.nanch, k = (u32)A.k, L = (u32)A.L;
    const u32 nchunks = (W + 63u) >> 6;
    for (u32 qb = 0; qb < nq; qb += KJ_EB) {
        const u32 nqb = min((u32)KJ_EB, nq - qb);
        // hits so far of the block's entry `lane` (the block holds 64 entries: one counter per lane, read with
        // v_readlane -- a counter in LDS behind a volatile pointer became a FLAT load +
        // store with a full wait in every iteration that had a hit)
        u32 cnt_reg = 0;
        // ---- stage the block, sorted by anchor ----------------------------------------------------------
        u32 segend[KJ_AMAX];
        {
            KJ_WAVE_SYNC();                       // (the previous block's readers are done)
            const bool valid = lane < nqb;
            const u32 e = valid ? A.ents[efirst + qb + lane] : 0u;
            const u32 p = e / nanch, a = e - p * nanch;
            u32 posn = 0, run = 0;
#pragma unroll
            for (int aa = 0; aa < KJ_AMAX; ++aa) {
                const unsigned long long m = __ballot(valid && a == (u32)aa);
                if (a == (u32)aa) posn = run + (u32)__popcll(m & lt);
                run += (u32)__popcll(m);
                segend[aa] = run;
            }
            if (valid) {
#pragma unroll
                for (int w = 0; w < NW; ++w) sm.img[posn * NW + w] = A.pplanes[(size_t)p * NW + w];
                sm.b[posn] = A.bucket_of ? A.bucket_of[p] : p;
                sm.eb[posn] = WRITE ? A.ebase[e] : e;
                sm.grp[posn] = A.probe_group ? A.probe_group[p] : 0;
            }
            KJ_WAVE_SYNC();
        }
        for (u32 c0 = 0; c0 < W; c0 += 64) {
            const bool inw = c0 + lane < W;
            u32 pos = 0, sq = 0, lo = 0, hi = 0, seg = 0;
            i32 sgrp = 0;
            unsigned long long mreg = 0;          // counting pass: the ballot of the block's entry `lane` in this chunk
            if (inw) {
                pos = (u32)A.hkey[i0 + c0 + lane];
                sq = A.hsq[i0 + c0 + lane];
                lo = A.seq_off[sq]; hi = A.seq_off[sq + 1];
                if (A.seq_group) sgrp = A.seq_group[sq];
                if (WRITE) seg = A.seq_genome ? (u32)A.seq_genome[sq] : sq;
            }
            u32 seg_lo = 0;
#pragma unroll
            for (int aa = 0; aa < KJ_AMAX; ++aa) {
                if (aa >= A.ntab) break;                       // wave-uniform
                const u32 seg_hi = segend[aa];
                if (seg_hi == seg_lo) continue;                // no entry of this anchor in the block
                const u32 o = pos - (u32)aa * k;
                const bool okw = inw && pos >= lo + (u32)aa * k && o + L <= hi;
                if (!__ballot(okw)) { seg_lo = seg_hi; continue; }
                KjWin<NW> win;
                kj_load_window<NW>(A.tq, okw ? o : 0u, win);
                u32 es = 0, ee = 0;
                if (WRITE) {
                    const u32 ge = o + L;
                    es = (o - lo > A.ext) ? o - A.ext : lo;
                    ee = (hi - ge > A.ext) ? ge + A.ext : hi;
                }
                // two entries per trip: two independent chains of LDS reads and bit work in flight
                auto test = [&](u32 j) -> bool {
                    u32 mw[NW];
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        const uint4 q = sm.img[j * NW + w];      // LDS broadcast
                        mw[w] = (win.x[w] ^ q.x) | (win.y[w] ^ q.y) | (win.z[w] ^ q.z);
                    }
                    mw[NW - 1] &= A.tailmask;
                    bool hit = okw & kj_accept<NW>(mw, (u32)aa, (int)k, A.mm);
                    if (A.probe_group) hit = hit & (sm.grp[j] == sgrp);
                    return hit;
                };
                auto file = [&](u32 j, bool hit) {
                    const unsigned long long hb = __ballot(hit);
                    if (hb) {
                        const u32 base = (u32)__builtin_amdgcn_readlane((int)cnt_reg, (int)j);
                        if (WRITE && hit) A.S[sm.eb[j] + base + (u32)__popcll(hb & lt)] = make_uint4(es, ee, seg, sm.b[j]);
                        if (lane == j) { cnt_reg = base + (u32)__popcll(hb); if (!WRITE) mreg = hb; }
                    }
                };
                u32 j = seg_lo;
                for (; j + 1 < seg_hi; j += 2) {
                    const bool h0 = test(j), h1 = test(j + 1);
                    file(j, h0);
                    file(j + 1, h1);
                }
                if (j < seg_hi) file(j, test(j));
                seg_lo = seg_hi;
            }
            if (!WRITE && mb != KJ_NOMASK) A.masks[(size_t)mb + ((size_t)(qb >> 6) * nchunks + (c0 >> 6)) * 64u + lane] = mreg;
        }
        if (!WRITE && lane < nqb) A.ecnt[sm.eb[lane]] = cnt_reg;
    }
}

// Short runs, one LANE per window (round 4, second half).  A wave-wide pass over a run costs a chain of dependent
// round trips whatever the run holds (entry ids -> images -> LDS; records -> bounds -> windows), which pays when the
// run is a biclique of hundreds of pairs and not when it is 6 windows x 2 entries -- and with insertions and
// deletions between strains (S4i) that is what most runs are: sibling strains no longer hold a probe's k-mer at
// the probe grid's phase, 60 % of all target positions hit the table, and a run is a few dozen windows of one
// k-mer against the one or two probes that carry it (count pass of S4i: 40 ms wave-wide).  Here the lanes of a
// wavefront are the windows of SEVERAL short runs -- every run that lies inside the chunk keeps its own lanes --
// and the entry loop runs to the longest entry list among them: lane l verifies entry j of ITS run; lanes of one
// run read the same entry and probe image (a handful of distinct lines per load), count by a ballot masked with the
// run's lanes, and write in lane = position order.  Every entry is still visited by exactly one wavefront.
// active: this lane holds a window; idx: its record; efirst / nq: its run's entries; runmask: the lanes of its run;
// leader: the run's lowest lane.
template <int NW, bool WRITE>
__device__ __forceinline__ void kj_lanes(const JoinArgs &A, bool active, u32 idx, u32 efirst, u32 nq,
                                         unsigned long long runmask, bool leader, u32 lane) {
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    const u32 k = (u32)A.k, L = (u32)A.L;
    u32 pos = 0, sq = 0, lo = 0, hi = 0;
    i32 sgrp = 0;
    if (active) {
        pos = (u32)A.hkey[idx];
        sq = A.hsq[idx];
        lo = A.seq_off[sq]; hi = A.seq_off[sq + 1];
        if (A.seq_group) sgrp = A.seq_group[sq];
    }
    u32 maxq = active ? nq : 0u;
    maxq = wave_max_all(maxq);
    for (u32 j = 0; j < maxq; ++j) {
        const bool on = active && j < nq;
        u32 e = 0, p = 0, a = 0;
        bool hit = false;
        if (on) {
            e = A.ents[efirst + j];
            p = (u32)(((unsigned long long)e * A.div_magic) >> 34);       // e / nanch (div_magic = ceil(2^34 / nanch), e < 2^31)
            a = e - p * (u32)A.nanch;
            bool ok = pos >= lo + a * k && pos - a * k + L <= hi;
            if (ok && A.probe_group) ok = A.probe_group[p] == sgrp;
            if (ok) {
                KjWin<NW> win;
                kj_load_window<NW>(A.tq, pos - a * k, win);
                u32 mw[NW];
#pragma unroll
                for (int x = 0; x < NW; ++x) {
                    const uint4 q = A.pplanes[(size_t)p * NW + x];
                    mw[x] = (win.x[x] ^ q.x) | (win.y[x] ^ q.y) | (win.z[x] ^ q.z);
                }
                mw[NW - 1] &= A.tailmask;
                hit = kj_accept<NW>(mw, a, (int)k, A.mm);
            }
        }
        const unsigned long long hb = __ballot(hit) & runmask;
        if (WRITE) {
            if (hit) A.S[A.ebase[e] + (u32)__popcll(hb & lt)] = kj_record(A, p, pos - a * k, sq, lo, hi);
        } else if (on && leader) {
            A.ecnt[e] = (u32)__popcll(hb);
        }
    }
}

// 3./4. a wavefront looks at 64 consecutive records of the sorted hit list and takes every run that STARTS there
//
// Round 12: ONE wavefront per workgroup (until then four).  Most wavefronts find no wave-wide run in their 64 records
// and are through at once, but in a workgroup of four their wave slots and the workgroup's LDS (4 KjLds) stayed taken
// until its one heavy wavefront had verified its runs: a CU held few heavy wavefronts, and those waited for their loads
// with nobody to issue in their place.  Alone, a wavefront gives back its 4,864 B (NW = 4) and its slot when it exits.
// S4, per step, counting + writing launch: 6.3 + 4.8 ms with four, 5.0 + 4.3 with two, 4.4 + 4.3 with one
// (DESIGN.md section 4 K1d, round 12; issuing the next window's loads ahead of the tests added nothing to that).
#define KJ_VERIFY_WAVES 1
template <int NW, bool WRITE>
__global__ void __launch_bounds__(64 * KJ_VERIFY_WAVES)
kj_verify_kernel(JoinArgs A) {
    __shared__ KjLds<NW> s_lds[KJ_VERIFY_WAVES];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 c64 = (blockIdx.x * (u32)KJ_VERIFY_WAVES + wave) * 64u;
    if (c64 >= A.nhit) return;                         // wave-uniform
    const u32 i = c64 + lane;
    const bool valid = i < A.nhit;
    const u32 slot = valid ? (u32)(A.hkey[i] >> 32) : 0xffffffffu;
    u32 prev = __shfl_up(slot, 1);
    if (lane == 0) prev = i ? (u32)(A.hkey[i - 1] >> 32) : 0xffffffffu;
    const bool head = valid && slot != prev;
    const unsigned long long hb = __ballot(head);
    u32 W = 0, Q = 0, first = 0;
    bool small = false;
    if (head) {
        const unsigned long long later = lane == 63 ? 0ull : (hb >> (lane + 1));
        if (later) {
            W = (u32)__ffsll((long long)later);
        } else {
            // the run reaches the end of this chunk: gallop on (the list is sorted by slot)
            u32 r = min(c64 + 64u, A.nhit), step = 1;
            while (r < A.nhit) {
                const u32 probe = (u32)min((unsigned long long)r + step - 1ull, (unsigned long long)A.nhit - 1ull);
                if ((u32)(A.hkey[probe] >> 32) == slot) { r = probe + 1u; if (step < (1u << 30)) step <<= 1; continue; }
                u32 lo_ = r, hi_ = probe;               // hkey[hi_] differs; first such index in [lo_, hi_]
                while (lo_ < hi_) {
                    const u32 mid = (lo_ + hi_) >> 1;
                    if ((u32)(A.hkey[mid] >> 32) == slot) lo_ = mid + 1u; else hi_ = mid;
                }
                r = lo_;
                break;
            }
            W = r - i;
        }
        const uint4 sl = A.slot[slot];
        first = sl.z; Q = sl.w;
        // short: its windows get lanes of their own (kj_lanes); the others a wave-wide pass each (kj_big)
        small = W < KJ_LANES_W && (unsigned long long)W * Q <= KJ_LANES_PAIRS;
    }
    if (!WRITE) {   // statistics: pairs verified, and the lane slots the wave-wide runs occupy (64 per chunk and entry)
        unsigned long long pr = (unsigned long long)W * Q;
        unsigned long long sl = (head && !small) ? (unsigned long long)((W + 63u) / 64u) * 64ull * Q : 0ull;
        wave_sum_n(pr, sl);
        // (64 shards each: an atomic on ONE address costs ~10 ns however it is issued, and a hit list of 10^8 records is 2 M wavefronts)
        if (lane == 0 && pr) { atomicAdd(&A.pairs[(c64 >> 6) & 63u], pr); if (sl) atomicAdd(&A.pairs[64u + ((c64 >> 6) & 63u)], sl); }
    }
    {
        // (a) the short runs that lie inside this chunk: every record of theirs is verified by its own lane
        const unsigned long long upto = hb & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        const int hl = upto ? 63 - __builtin_clzll(upto) : 0;            // my run's head lane (if it is headed here)
        const u32 hW = (u32)__shfl((int)W, hl), hQ = (u32)__shfl((int)Q, hl), hF = (u32)__shfl((int)first, hl);
        const bool hS = __shfl((int)small, hl) != 0;
        const bool inside = valid && upto != 0ull && hS && (u32)hl + hW <= 64u && lane < (u32)hl + hW;
        const unsigned long long rm = hW >= 64u ? ~0ull : (((1ull << hW) - 1ull) << hl);
        if (__ballot(inside)) kj_lanes<NW, WRITE>(A, inside, i, hF, hQ, rm, lane == (u32)hl, lane);
        // (b) the one short run that starts here and runs on into the next chunk: lanes 0 .. W - 1
        const unsigned long long cross = __ballot(head && small && lane + W > 64u);
        if (cross) {
            const int cl = __ffsll((long long)cross) - 1;
            const u32 cW = (u32)__builtin_amdgcn_readlane((int)W, cl), cQ = (u32)__builtin_amdgcn_readlane((int)Q, cl);
            const u32 cF = (u32)__builtin_amdgcn_readlane((int)first, cl), ci = (u32)__builtin_amdgcn_readlane((int)i, cl);
            kj_lanes<NW, WRITE>(A, lane < cW, ci + lane, cF, cQ, cW >= 64u ? ~0ull : ((1ull << cW) - 1ull), lane == 0, lane);
        }
    }
    unsigned long long bb = __ballot(head && !small);
    while (bb) {
        const int src = __ffsll((long long)bb) - 1;
        bb &= bb - 1;
        const u32 bi = (u32)__builtin_amdgcn_readlane((int)i, src), bW = (u32)__builtin_amdgcn_readlane((int)W, src);
        const u32 bf = (u32)__builtin_amdgcn_readlane((int)first, src), bQ = (u32)__builtin_amdgcn_readlane((int)Q, src);
        if ((unsigned long long)bW * bQ > KJ_GIANT_PAIRS) {
            if (!WRITE) {   // (the writing pass finds the tasks where the counting pass left them)
                const u32 qsub = max(1u, KJ_GIANT_PAIRS / bW), nt = (bQ + qsub - 1u) / qsub;
                u32 g0 = 0;
                if (lane == 0) g0 = atomicAdd(A.giant_n, nt);
                g0 = (u32)__builtin_amdgcn_readfirstlane((int)g0);
                for (u32 j = lane; j < nt; j += 64)
                    if (g0 + j < A.giant_cap) A.giant[g0 + j] = make_uint4(bi, bW, bf + j * qsub, min(qsub, bQ - j * qsub));
            }
            continue;
        }
        u32 mb = KJ_NOMASK;
        if (A.masks) {
            if (!WRITE) {
                const u32 need = ((bQ + 63u) >> 6) * ((bW + 63u) >> 6) * 64u;
                if (lane == 0) {
                    const u32 part = (c64 >> 6) & 63u, pcap = A.mask_cap >> 6;                      // this chunk's part of the store
                    const unsigned long long at = atomicAdd(A.mcursor + part, (unsigned long long)need);   // (64 bits: never wraps)
                    mb = at + need <= (unsigned long long)pcap ? part * pcap + (u32)at : KJ_NOMASK;       // full: this run is verified twice
                    A.mbase[bi] = mb;
                }
                mb = (u32)__builtin_amdgcn_readfirstlane((int)mb);
            } else mb = A.mbase[bi];
        }
        kj_big<NW, WRITE>(A, s_lds[wave], bi, bW, bf, bQ, mb, lane);
    }
}

// the tasks of the runs that were cut by entries
template <int NW, bool WRITE>
__global__ void __launch_bounds__(256)
kj_giant_kernel(JoinArgs A) {
    __shared__ KjLds<NW> s_lds[4];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 n = min(*A.giant_n, A.giant_cap);
    // tasks are handed out one at a time (cursor: giant_n[1] in the counting pass, [2] in the writing pass):
    // they differ in length by orders of magnitude
    for (;;) {
        u32 t = 0;
        if (lane == 0) t = atomicAdd(A.giant_n + (WRITE ? 2 : 1), 1u);
        t = (u32)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= n) break;
        const uint4 tk = A.giant[t];
        const u32 tW = (u32)__builtin_amdgcn_readfirstlane((int)tk.y), tQ = (u32)__builtin_amdgcn_readfirstlane((int)tk.w);
        u32 mb = KJ_NOMASK;
        if (A.masks) {
            if (!WRITE) {
                const u32 need = ((tQ + 63u) >> 6) * ((tW + 63u) >> 6) * 64u;
                if (lane == 0) {
                    const u32 part = t & 63u, pcap = A.mask_cap >> 6;
                    const unsigned long long at = atomicAdd(A.mcursor + part, (unsigned long long)need);
                    mb = at + need <= (unsigned long long)pcap ? part * pcap + (u32)at : KJ_NOMASK;
                    A.gmbase[t] = mb;
                }
                mb = (u32)__builtin_amdgcn_readfirstlane((int)mb);
            } else mb = A.gmbase[t];
        }
        kj_big<NW, WRITE>(A, s_lds[wave],
                          (u32)__builtin_amdgcn_readfirstlane((int)tk.x), tW,
                          (u32)__builtin_amdgcn_readfirstlane((int)tk.z), tQ, mb, lane);
    }
}

// hits per bucket from the hits per entry (a bucket = the probes of one set id; usually one)
__global__ void __launch_bounds__(256)
kj_bucket_count_kernel(const u32 *__restrict__ ecnt, u32 nprobes, int nanch, int ntab, const u32 *__restrict__ bucket_of,
                       u32 *__restrict__ bcnt) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nprobes) return;
    u32 tot = 0;
    for (int a = 0; a < ntab; ++a) tot += ecnt[(size_t)p * nanch + a];
    if (tot) atomicAdd(&bcnt[bucket_of ? bucket_of[p] : p], tot);
}

// every entry's first record: the probe's share of its bucket (a cursor per bucket when buckets hold several
// probes), its anchors one after the other
__global__ void __launch_bounds__(256)
kj_bases_kernel(const u32 *__restrict__ ecnt, u32 nprobes, int nanch, int ntab, const u32 *__restrict__ bucket_of,
                const u32 *__restrict__ bstart, u32 *__restrict__ bcur, u32 *__restrict__ ebase) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nprobes) return;
    u32 tot = 0;
    for (int a = 0; a < ntab; ++a) tot += ecnt[(size_t)p * nanch + a];
    if (!tot) return;
    const u32 b = bucket_of ? bucket_of[p] : p;
    u32 base = bstart[b] + (bucket_of ? atomicAdd(&bcur[b], tot) : 0u);
    for (int a = 0; a < ntab; ++a) { ebase[(size_t)p * nanch + a] = base; base += ecnt[(size_t)p * nanch + a]; }
}

typedef void (*kj_kernel_fn)(JoinArgs);
template <bool WRITE> static kj_kernel_fn pick_kj_verify(int nw) { PICK_NW(8, nw, kj_verify_kernel, WRITE); }
template <bool WRITE> static kj_kernel_fn pick_kj_giant(int nw) { PICK_NW(8, nw, kj_giant_kernel, WRITE); }
