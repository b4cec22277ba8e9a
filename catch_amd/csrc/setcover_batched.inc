// Batched ("frontier") greedy solver (included by setcover.hip).
//
// Used when every universe must be fully covered (universe_p == 1 for all,
// so min(left, count) never binds and gain(s) = number of still-uncovered
// elements of s).  Rows of at most 257 bases (<= 5 bitmap words) take the
// gf_* kernels, longer ones the gfl_* kernels further down.
//
// Why many picks per round are exact.  Order all sets of the current rank by
// the packed key (gain << 32) | (0xFFFFFFFF - id) (larger = picked earlier; keys
// are distinct).  Let c be a set whose key is larger than the key of EVERY
// other set that shares a still-uncovered element with it.  The sequential
// greedy (catch/utils/set_cover.py:448-613) changes gain(c) only by picking a
// set that overlaps c; all of those have smaller keys, keys never grow, so c
// reaches the top with its gain unchanged and IS picked, before any set that
// overlaps it -- and a universe cannot become fully covered (the stop
// condition with p == 1) while c still has uncovered elements.  Picking c now
// instead of later changes nothing else: the sets it affects are evaluated
// after it either way, and sets with larger keys do not overlap it.  Hence
// taking ALL such "locally maximal" sets at once yields exactly the picks of
// the sequential algorithm.  The sequential algorithm picks in descending key
// order (gains never grow and the maximum is taken each time), and a locally
// maximal set is picked with the key it has now, so sorting the picks of a rank
// by the key they were accepted with restores the sequential pick order.
//
// A round is two grid-wide launches over the LIVE sets (gain > 0, not picked);
// a group of 16 lanes owns one set and walks its rows:
//
//  gf_count_claim_kernel
//     re-counts every row of the set against the bitmap (all word loads of a
//     row issued together), stores which of its words still hold uncovered
//     bits (rowflag), sums and stores the gain and -- when the set has the
//     current rank -- raises owner[word] to
//     its key with atomicMax for every such word (word granularity is a
//     conservative overlap test).
//     Losers are marked in the same launch (lost[s] = round tag): by
//     themselves when they find or are handed back a larger key, by the set
//     that displaces them otherwise.
//  gf_check_apply_kernel
//     a set that claimed is accepted iff it owns all its words, i.e. it was not
//     marked.  The global maximum always is, so every round makes progress.
//     Accepted sets clear their bits and are recorded with their key.  The kernel also zeroes the
//     other owner buffer (rounds alternate between two) and thread 0 advances
//     the rank when no set of the current rank had anything left to cover
//     (set_cover.py:522-526).
//
// Rows that are fully covered stay so: their rowflag is 0 and later rounds
// skip their bitmap words.
//
// Cross-kernel visibility is all the rounds need: the bitmap is modified by
// atomicAnd in check+apply and read in the NEXT launch, the owner words are
// raised by atomicMax in count+claim and read in the next launch, so plain
// (L2-cached) loads are correct; agent-scope (sc1) loads of the same words cost
// 20 % more per round on S2 and 25 % more at S4 (every load a fabric
// transaction).  The look at the current owner inside count+claim may be
// stale, which only costs a redundant atomic.
#define GF_THREADS 256
// lanes per set: 16 when sets have a handful of rows (S2: 9), a whole
// wavefront when they have dozens to thousands (one row per genome hit)

struct FrontArgs {
    unsigned long long *bm;
    unsigned long long *owner[2];   // per bitmap word: largest key claiming it this round
    const uint2 *frow;              // rows in set order: {gs, ge} (8 B: the first rounds stream every row)
    const i32 *row_univ;            // universe of a row (read only when a row is applied)
    const u32 *set_ptr, *rank;
    u32 *usize;                     // elements of the universe still to cover
    u32 *gain, *claimed, *picked, *picks;
    u32 *lost;                      // round + 1 when the set lost a word in that round (gf_* kernels)
    unsigned long long *pick_key;
    u8 *rowflag;                    // bit t: word t of the row holds uncovered bits
    unsigned long long *blkcnt;     // per workgroup: rows re-counted, words read (work counters)
    // Large instances only (null otherwise): the live sets of a round, built by
    // the previous round's check+apply launch.  With millions of sets of which
    // a few per cent stay alive, walking all of them cost a dependent load pair
    // per dead set (S4: 240 sets per wavefront, ~360 us per round).
    u32 *live[2];
    GreedyState *st;
    u32 nsets, nwords;
};
#define GF_LIST_TILE 4096   // sets per workgroup step of the list build: one cursor atomic each

// No same-address atomics in the round kernels: ~10 ns each on MI355X, a
// per-wavefront counter update alone cost 75 us per launch.  Dead sets are
// skipped by their stored gain instead of being compacted away, the "some set
// of this rank claimed" signal is a plain store, work counters are per
// workgroup.
template <int G>
__global__ void __launch_bounds__(GF_THREADS)
gf_count_claim_kernel(FrontArgs a, u32 round) {
    constexpr u32 GF_GROUP = G, GF_SETS = GF_THREADS / G;
    __shared__ u32 s_claim, s_rows, s_words;
    GreedyState *st = a.st;
    if (st->done || st->n_need == 0) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) st->iters = round + 1;
    if (threadIdx.x == 0) { s_claim = 0; s_rows = 0; s_words = 0; }
    __syncthreads();
    const u32 par = round & 1;
    const u32 cur_rank = st->cur_rank;
    const u32 sub = threadIdx.x & (GF_GROUP - 1), grp = threadIdx.x / GF_GROUP;
    unsigned long long *owner = a.owner[par];
    u32 cnt_rows = 0, cnt_words = 0;
    bool any_claim = false;
    const bool listed = a.live[0] != nullptr && round > 0;
    const u32 nwork = listed ? st->fr_live[par] : a.nsets;
    if (blockIdx.x == 0 && threadIdx.x == 0) st->fr_live[par ^ 1] = 0;   // filled by this round's check+apply
    for (u32 li = blockIdx.x * GF_SETS + grp; li < nwork; li += gridDim.x * GF_SETS) {
        const u32 s = listed ? a.live[par][li] : li;
        // everything that only depends on s is requested at once: a launch is a
        // chain of dependent memory round trips (~2 us each right after a kernel
        // boundary), and on small instances their number IS the run time
        const u32 pk = a.picked[s], g0 = a.gain[s], r0 = a.set_ptr[s], r1 = a.set_ptr[s + 1], rk = a.rank[s];
        if (pk || (round && g0 == 0)) continue;   // chosen, or nothing left to offer
        u32 cnt = 0;
        u32 fl_first = 0, w0_first = 0;           // first row of this lane: kept for the claim loop
        for (u32 j = r0 + sub, it = 0; j < r1; j += GF_GROUP, ++it) {
            const u32 oldfl = round ? (u32)a.rowflag[j] : 1u;
            const uint2 wr = a.frow[j];
            if (oldfl == 0) continue;   // fully covered earlier
            const u32 x = wr.x, e = wr.y;
            const u32 w0 = x >> 6, nwd = ((e - 1) >> 6) - w0 + 1;
            const u64 m0 = ~0ull << (x & 63), m1 = ~0ull >> (63 - ((e - 1) & 63));
            u32 fl = 0;
            if (round == 0) {
                // nothing is covered yet and the universe is the union of the rows:
                // every base of the row counts, no need to look at the bitmap
                cnt += e - x;
                fl = (1u << nwd) - 1u;
            } else {
                unsigned long long v[RP_MAXW];
                load_words5(a.bm + w0, v, oldfl);   // unflagged words: covered for this row
#pragma unroll
                for (u32 t = 0; t < RP_MAXW; ++t) {
                    u64 m = ~0ull;
                    if (t == 0) m &= m0;
                    if (t == nwd - 1) m &= m1;
                    const u64 um = t < nwd ? (v[t] & m) : 0ull;
                    cnt += (u32)__popcll(um);
                    fl |= um ? (1u << t) : 0u;
                }
            }
            a.rowflag[j] = (u8)fl;
            if (it == 0) { fl_first = fl; w0_first = w0; }
            cnt_rows++;
            cnt_words += nwd;
        }
        cnt = group_sum<G>(cnt);
        if (sub == 0) a.gain[s] = cnt;
        if (cnt == 0 || rk != cur_rank) continue;
        any_claim = true;
        const unsigned long long key = ((unsigned long long)cnt << ID_BITS) | (unsigned long long)(ID_MASK - s);
        bool lost = false;
        for (u32 j = r0 + sub, it = 0; j < r1; j += GF_GROUP, ++it) {
            const u32 fl = it == 0 ? fl_first : (u32)a.rowflag[j];
            if (!fl) continue;
            const u32 w0 = it == 0 ? w0_first : a.frow[j].x >> 6;
            // owner words only grow during a launch: a word already seen above
            // this key cannot be won (even in a stale view), which spares most of
            // the atomics.  Who loses is settled here: a larger key found, or handed
            // back by the atomicMax, marks this set; a smaller one handed back marks
            // the set it belonged to -- after the launch exactly the sets that hold
            // every word they claimed are unmarked.
            unsigned long long seen[RP_MAXW];
            load_words5(owner + w0, seen, fl);   // owner has slack words
#pragma unroll
            for (u32 t = 0; t < RP_MAXW; ++t) {
                if (!(fl & (1u << t))) continue;
                unsigned long long other = seen[t];
                if (other < key) other = atomicMax(&owner[w0 + t], key);
                if (other > key) lost = true;
                else if (other && other < key) a.lost[ID_MASK - (u32)other] = round + 1;
            }
        }
        if (lost) a.lost[s] = round + 1;
        if (sub == 0) a.claimed[s] = round + 1;
    }
    wave_sum_n(cnt_rows, cnt_words);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&s_rows, cnt_rows); atomicAdd(&s_words, cnt_words); }
    if (any_claim && sub == 0) s_claim = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_claim) st->fr_claim[par] = 1;
        a.blkcnt[2 * blockIdx.x] += s_rows;
        a.blkcnt[2 * blockIdx.x + 1] += s_words;
    }
}

template <int G>
__global__ void __launch_bounds__(GF_THREADS)
gf_check_apply_kernel(FrontArgs a, u32 round) {
    constexpr u32 GF_GROUP = G, GF_SETS = GF_THREADS / G;
    GreedyState *st = a.st;
    const u32 par = round & 1;
    const u32 sub = threadIdx.x & (GF_GROUP - 1), grp = threadIdx.x / GF_GROUP;
    // the other owner buffer serves the next round
    for (u32 i = blockIdx.x * GF_THREADS + threadIdx.x; i < a.nwords; i += gridDim.x * GF_THREADS)
        a.owner[par ^ 1][i] = 0ull;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const u32 claimed = st->fr_claim[par];
        st->fr_claim[par ^ 1] = 0;
        // nothing claimed: nothing is applied in this launch, n_need is stable
        if (claimed == 0 && !st->done && st->n_need) {
            // no set of this rank covers anything still needed: next rank
            const u32 nr = st->cur_rank + 1;
            st->cur_rank = nr;
            if (nr >= st->nrank) st->done = 2;
        }
    }
    if (a.live[0] != nullptr) {
        // next round's live list: not chosen so far, something left to offer after
        // this round's count (sets chosen in THIS launch drop out at their next
        // visit).  One thread per set, one cursor atomic per GF_LIST_TILE sets.
        __shared__ u32 s_cnt[GF_THREADS / 64], s_base;
        u32 *out = a.live[par ^ 1];
        for (u32 t0 = blockIdx.x * GF_LIST_TILE; t0 < a.nsets; t0 += gridDim.x * GF_LIST_TILE) {
            constexpr int PER = GF_LIST_TILE / GF_THREADS;
            u32 mask = 0, mine = 0;
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const u32 s = t0 + q * GF_THREADS + threadIdx.x;
                const bool lv = s < a.nsets && a.gain[s] != 0 && !a.picked[s];
                mask |= lv ? (1u << q) : 0u;
                mine += lv ? 1u : 0u;
            }
            const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
            const u32 inc = wave_incl_scan(mine, (int)lane);
            __syncthreads();
            if (lane == 63) s_cnt[wave] = inc;
            __syncthreads();
            u32 woff = 0, tot = 0;
            for (int w = 0; w < GF_THREADS / 64; ++w) { if (w < (int)wave) woff += s_cnt[w]; tot += s_cnt[w]; }
            if (threadIdx.x == 0) s_base = tot ? atomicAdd(&st->fr_live[par ^ 1], tot) : 0u;
            __syncthreads();
            u32 o = s_base + woff + inc - mine;
#pragma unroll
            for (int q = 0; q < PER; ++q)
                if (mask & (1u << q)) out[o++] = t0 + q * GF_THREADS + threadIdx.x;
        }
    }
    u32 cnt_rows = 0;
    const bool listed = a.live[0] != nullptr && round > 0;
    const u32 nwork = listed ? st->fr_live[par] : a.nsets;
    for (u32 li = blockIdx.x * GF_SETS + grp; li < nwork; li += gridDim.x * GF_SETS) {
        const u32 s = listed ? a.live[par][li] : li;
        const u32 cl = a.claimed[s], ls = a.lost[s], r0 = a.set_ptr[s], r1 = a.set_ptr[s + 1], g0 = a.gain[s];
        if (cl != round + 1 || ls == round + 1) continue;
        const unsigned long long key = ((unsigned long long)g0 << ID_BITS) | (unsigned long long)(ID_MASK - s);
        // accepted (it holds every word it claimed): clear the bits, credit the universes
        for (u32 j = r0 + sub; j < r1; j += GF_GROUP) {
            const u32 fl = a.rowflag[j];
            if (!fl) continue;
            const uint2 wr = a.frow[j];
            const u32 x = wr.x, e = wr.y;
            const u32 w0 = x >> 6, nwd = ((e - 1) >> 6) - w0 + 1;
            const u64 m0 = ~0ull << (x & 63), m1 = ~0ull >> (63 - ((e - 1) & 63));
            u32 cleared = 0;
#pragma unroll
            for (u32 t = 0; t < RP_MAXW; ++t) {
                if (!(fl & (1u << t))) continue;
                u64 m = ~0ull;
                if (t == 0) m &= m0;
                if (t == nwd - 1) m &= m1;
                cleared += (u32)__popcll(atomicAnd(&a.bm[w0 + t], ~m) & m);
            }
            a.rowflag[j] = 0;
            cnt_rows++;
            if (cleared) {
                // can == 0 everywhere: the need of a universe is its size
                const u32 before = atomicSub(&a.usize[a.row_univ[j]], cleared);
                if (before == cleared) atomicSub(&st->n_need, 1u);
            }
        }
        if (sub == 0) {
            const u32 slot = atomicAdd(&st->npicks, 1u);
            a.picks[slot] = s;
            a.pick_key[slot] = key;
            a.picked[s] = 1u;
        }
    }
    (void)cnt_rows;
}

// Round kernels for rows of ANY length (gfl_*; used when a row exceeds 257
// bases, e.g. -e 100 at -pl 100).  A group of G lanes (16 or 64) owns one
// set; inside it 8 consecutive lanes own one ROW and lane `sub` of them owns
// the row's bitmap / owner words sub, sub+8, ... (a row of <= 449 bases has at
// most 8 words, so one step).  A wave-level load of bitmap or owner words then
// covers G/8 rows per set x ONE contiguous run of <= 64 bytes per row, and the
// word loop takes rows of any length.  Measured against the lane-per-row
// kernels above on S4 (rows of <= 250 bases, where both apply): 203 vs 127 ms
// per step -- eight times the wave-level instructions per row cost more than
// the 4x fewer cache-line look-ups save -- so these are the fallback for long
// rows only (before them such instances ran on ONE workgroup).
//
// rowflag[j], bit s: some word t = s (mod 8) of the row still holds uncovered
// bits of the row (exact per word for rows of <= 8 words, conservative for
// longer ones: claiming a word without uncovered bits only blocks more).
//
// No same-address atomics in the round kernels: ~10 ns each on MI355X, a
// per-wavefront counter update alone cost 75 us per launch.  Dead sets are
// skipped by their stored gain instead of being compacted away, the "some set
// of this rank claimed" signal is a plain store, work counters are per
// workgroup.
// mask of the bits of [x, e) inside bitmap word w0 + t
__device__ __forceinline__ u64 row_word_mask(u32 x, u32 e, u32 t, u32 nwd) {
    u64 m = ~0ull;
    if (t == 0) m &= ~0ull << (x & 63);
    if (t == nwd - 1) m &= ~0ull >> (63 - ((e - 1) & 63));
    return m;
}

template <int G>
__global__ void __launch_bounds__(GF_THREADS)
gfl_count_claim_kernel(FrontArgs a, u32 round) {
    constexpr u32 GF_SETS = GF_THREADS / G, RPI = G / 8;   // sets per workgroup, rows per step of a group
    constexpr u32 UNR = G == 64 ? 4 : 8;                   // row steps in flight per lane
    __shared__ u32 s_claim, s_rows, s_words;
    GreedyState *st = a.st;
    if (st->done || st->n_need == 0) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) st->iters = round + 1;
    if (threadIdx.x == 0) { s_claim = 0; s_rows = 0; s_words = 0; }
    __syncthreads();
    const u32 par = round & 1;
    const u32 cur_rank = st->cur_rank;
    const u32 lig = threadIdx.x & (G - 1), grp = threadIdx.x / G;
    const u32 sub = lig & 7, rsl = lig >> 3;           // word lane, row slot inside the group
    const u32 bsh = (threadIdx.x & 63) & ~7u;          // where this row's 8 lanes sit in a ballot
    unsigned long long *owner = a.owner[par];
    u32 cnt_rows = 0, cnt_words = 0;
    bool any_claim = false;
    const bool listed = a.live[0] != nullptr && round > 0;
    const u32 nwork = listed ? st->fr_live[par] : a.nsets;
    if (blockIdx.x == 0 && threadIdx.x == 0) st->fr_live[par ^ 1] = 0;   // filled by this round's check+apply
    for (u32 li = blockIdx.x * GF_SETS + grp; li < nwork; li += gridDim.x * GF_SETS) {
        const u32 s = listed ? a.live[par][li] : li;
        // everything that only depends on s is requested at once: a launch is a
        // chain of dependent memory round trips (~2 us each right after a kernel
        // boundary), and on small instances their number IS the run time
        const u32 pk = a.picked[s], g0 = a.gain[s], r0 = a.set_ptr[s], r1 = a.set_ptr[s + 1], rk = a.rank[s];
        if (pk || (round && g0 == 0)) continue;   // chosen, or nothing left to offer
        u32 cnt = 0;
        u32 fl_first[UNR];                        // first step of this row slot: kept for the claim loop
        uint2 wr_first[UNR];
#pragma unroll
        for (u32 u = 0; u < UNR; ++u) { fl_first[u] = 0; wr_first[u] = make_uint2(0, 1); }
        // UNR row steps at a time, every load of a step issued before the first
        // use: a set is a chain of dependent round trips (row record -> bitmap
        // word), and with 8 lanes per row a set takes 8x the steps it took with
        // a lane per row -- without the unrolling the rounds were latency-bound
        // (S4: 127 -> 276 ms per step)
        for (u32 j0 = r0 + rsl, it = 0; j0 < r1; j0 += UNR * RPI, ++it) {
            u32 oldfl[UNR];
            uint2 wr[UNR];
#pragma unroll
            for (u32 u = 0; u < UNR; ++u) {
                const u32 j = j0 + u * RPI;
                const bool in = j < r1;
                oldfl[u] = in ? (round ? (u32)a.rowflag[j] : 0xffu) : 0u;
                wr[u] = in ? a.frow[j] : make_uint2(0, 1);
            }
            u64 v[UNR];
#pragma unroll
            for (u32 u = 0; u < UNR; ++u) {
                const u32 w0 = wr[u].x >> 6, nwd = ((wr[u].y - 1) >> 6) - w0 + 1;
                v[u] = (round && (oldfl[u] & (1u << sub)) && sub < nwd) ? a.bm[w0 + sub] : 0ull;
            }
#pragma unroll
            for (u32 u = 0; u < UNR; ++u) {
                const u32 j = j0 + u * RPI;
                if (it == 0) wr_first[u] = wr[u];
                if (oldfl[u] == 0) continue;   // fully covered earlier (or past the set's rows)
                const u32 x = wr[u].x, e = wr[u].y;
                const u32 w0 = x >> 6, nwd = ((e - 1) >> 6) - w0 + 1;
                bool alive = false;
                if (round == 0) {
                    // nothing is covered yet and the universe is the union of the rows:
                    // every base of the row counts, no need to look at the bitmap
                    if (sub == 0) cnt += e - x;
                    alive = sub < nwd;
                } else if (oldfl[u] & (1u << sub)) {
                    if (sub < nwd) {
                        const u64 um = v[u] & row_word_mask(x, e, sub, nwd);
                        cnt += (u32)__popcll(um);
                        alive = um != 0;
                        cnt_words++;
                    }
                    for (u32 t = sub + 8; t < nwd; t += 8) {   // rows of more than 8 words
                        const u64 um = a.bm[w0 + t] & row_word_mask(x, e, t, nwd);
                        cnt += (u32)__popcll(um);
                        alive = alive || um != 0;
                        cnt_words++;
                    }
                }
                const u32 fl = (u32)(__ballot(alive) >> bsh) & 0xffu;
                if (sub == 0) { a.rowflag[j] = (u8)fl; cnt_rows++; }
                if (it == 0) fl_first[u] = fl;
            }
        }
        cnt = group_sum<G>(cnt);
        if (lig == 0) a.gain[s] = cnt;
        if (cnt == 0 || rk != cur_rank) continue;
        any_claim = true;
        const unsigned long long key = ((unsigned long long)cnt << ID_BITS) | (unsigned long long)(ID_MASK - s);
        for (u32 j0 = r0 + rsl, it = 0; j0 < r1; j0 += UNR * RPI, ++it) {
            u32 fl[UNR];
            uint2 wr[UNR];
#pragma unroll
            for (u32 u = 0; u < UNR; ++u) {
                const u32 j = j0 + u * RPI;
                const bool in = j < r1;
                fl[u] = it == 0 ? fl_first[u] : (in ? (u32)a.rowflag[j] : 0u);
                wr[u] = it == 0 ? wr_first[u] : (in ? a.frow[j] : make_uint2(0, 1));
            }
            // owner words only grow during a launch: a word already seen above
            // this key cannot be won, which spares most of the atomics (a stale
            // view only costs an atomic)
            unsigned long long seen[UNR];
#pragma unroll
            for (u32 u = 0; u < UNR; ++u) {
                const u32 w0 = wr[u].x >> 6, nwd = ((wr[u].y - 1) >> 6) - w0 + 1;
                seen[u] = ((fl[u] & (1u << sub)) && sub < nwd) ? owner[w0 + sub] : ~0ull;
            }
#pragma unroll
            for (u32 u = 0; u < UNR; ++u) {
                if (!(fl[u] & (1u << sub))) continue;
                const u32 w0 = wr[u].x >> 6, nwd = ((wr[u].y - 1) >> 6) - w0 + 1;
                if (seen[u] < key) atomicMax(&owner[w0 + sub], key);
                for (u32 t = sub + 8; t < nwd; t += 8)
                    if (owner[w0 + t] < key) atomicMax(&owner[w0 + t], key);
            }
        }
        if (lig == 0) a.claimed[s] = round + 1;
    }
    wave_sum_n(cnt_rows, cnt_words);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&s_rows, cnt_rows); atomicAdd(&s_words, cnt_words); }
    if (any_claim && lig == 0) s_claim = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_claim) st->fr_claim[par] = 1;
        a.blkcnt[2 * blockIdx.x] += s_rows;
        a.blkcnt[2 * blockIdx.x + 1] += s_words;
    }
}

template <int G>
__global__ void __launch_bounds__(GF_THREADS)
gfl_check_apply_kernel(FrontArgs a, u32 round) {
    constexpr u32 GF_SETS = GF_THREADS / G, RPI = G / 8;
    constexpr u32 UNR = G == 64 ? 4 : 8;
    GreedyState *st = a.st;
    const u32 par = round & 1;
    const u32 lig = threadIdx.x & (G - 1), grp = threadIdx.x / G;
    const u32 sub = lig & 7, rsl = lig >> 3;
    const unsigned long long *owner = a.owner[par];
    // the other owner buffer serves the next round
    for (u32 i = blockIdx.x * GF_THREADS + threadIdx.x; i < a.nwords; i += gridDim.x * GF_THREADS)
        a.owner[par ^ 1][i] = 0ull;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const u32 claimed = st->fr_claim[par];
        st->fr_claim[par ^ 1] = 0;
        // nothing claimed: nothing is applied in this launch, n_need is stable
        if (claimed == 0 && !st->done && st->n_need) {
            // no set of this rank covers anything still needed: next rank
            const u32 nr = st->cur_rank + 1;
            st->cur_rank = nr;
            if (nr >= st->nrank) st->done = 2;
        }
    }
    if (a.live[0] != nullptr) {
        // next round's live list: not chosen so far, something left to offer after
        // this round's count (sets chosen in THIS launch drop out at their next
        // visit).  One thread per set, one cursor atomic per GF_LIST_TILE sets.
        __shared__ u32 s_cnt[GF_THREADS / 64], s_base;
        u32 *out = a.live[par ^ 1];
        for (u32 t0 = blockIdx.x * GF_LIST_TILE; t0 < a.nsets; t0 += gridDim.x * GF_LIST_TILE) {
            constexpr int PER = GF_LIST_TILE / GF_THREADS;
            u32 mask = 0, mine = 0;
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const u32 s = t0 + q * GF_THREADS + threadIdx.x;
                const bool lv = s < a.nsets && a.gain[s] != 0 && !a.picked[s];
                mask |= lv ? (1u << q) : 0u;
                mine += lv ? 1u : 0u;
            }
            const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
            const u32 inc = wave_incl_scan(mine, (int)lane);
            __syncthreads();
            if (lane == 63) s_cnt[wave] = inc;
            __syncthreads();
            u32 woff = 0, tot = 0;
            for (int w = 0; w < GF_THREADS / 64; ++w) { if (w < (int)wave) woff += s_cnt[w]; tot += s_cnt[w]; }
            if (threadIdx.x == 0) s_base = tot ? atomicAdd(&st->fr_live[par ^ 1], tot) : 0u;
            __syncthreads();
            u32 o = s_base + woff + inc - mine;
#pragma unroll
            for (int q = 0; q < PER; ++q)
                if (mask & (1u << q)) out[o++] = t0 + q * GF_THREADS + threadIdx.x;
        }
    }
    const bool listed = a.live[0] != nullptr && round > 0;
    const u32 nwork = listed ? st->fr_live[par] : a.nsets;
    for (u32 li = blockIdx.x * GF_SETS + grp; li < nwork; li += gridDim.x * GF_SETS) {
        const u32 s = listed ? a.live[par][li] : li;
        const u32 cl = a.claimed[s], r0 = a.set_ptr[s], r1 = a.set_ptr[s + 1], g0 = a.gain[s];
        if (cl != round + 1) continue;
        const unsigned long long key = ((unsigned long long)g0 << ID_BITS) | (unsigned long long)(ID_MASK - s);
        u32 lost = 0;
        u32 fl_first[UNR];
        uint2 wr_first[UNR];
#pragma unroll
        for (u32 u = 0; u < UNR; ++u) { fl_first[u] = 0; wr_first[u] = make_uint2(0, 1); }
        for (u32 j0 = r0 + rsl, it = 0; j0 < r1; j0 += UNR * RPI, ++it) {
            u32 fl[UNR];
            uint2 wr[UNR];
#pragma unroll
            for (u32 u = 0; u < UNR; ++u) {
                const u32 j = j0 + u * RPI;
                const bool in = j < r1;
                fl[u] = in ? (u32)a.rowflag[j] : 0u;
                wr[u] = in ? a.frow[j] : make_uint2(0, 1);
            }
            unsigned long long ow[UNR];
#pragma unroll
            for (u32 u = 0; u < UNR; ++u) {
                const u32 w0 = wr[u].x >> 6, nwd = ((wr[u].y - 1) >> 6) - w0 + 1;
                ow[u] = ((fl[u] & (1u << sub)) && sub < nwd) ? owner[w0 + sub] : key;
            }
#pragma unroll
            for (u32 u = 0; u < UNR; ++u) {
                if (it == 0) { fl_first[u] = fl[u]; wr_first[u] = wr[u]; }
                if (ow[u] != key) lost = 1;
                if (fl[u] & (1u << sub)) {
                    const u32 w0 = wr[u].x >> 6, nwd = ((wr[u].y - 1) >> 6) - w0 + 1;
                    for (u32 t = sub + 8; t < nwd; t += 8)
                        if (owner[w0 + t] != key) lost = 1;
                }
            }
        }
        lost = group_sum<G>(lost);
        if (lost) continue;
        // accepted: clear the bits, credit the universes
        for (u32 j0 = r0 + rsl, it = 0; j0 < r1; j0 += UNR * RPI, ++it) {
#pragma unroll
            for (u32 u = 0; u < UNR; ++u) {
                const u32 j = j0 + u * RPI;
                const u32 fl = it == 0 ? fl_first[u] : (j < r1 ? (u32)a.rowflag[j] : 0u);
                if (!fl) continue;                       // the 8 lanes of a row agree
                const uint2 wr = it == 0 ? wr_first[u] : a.frow[j];
                const u32 x = wr.x, e = wr.y;
                const u32 w0 = x >> 6, nwd = ((e - 1) >> 6) - w0 + 1;
                u32 cleared = 0;
                if (fl & (1u << sub))
                    for (u32 t = sub; t < nwd; t += 8) {
                        const u64 m = row_word_mask(x, e, t, nwd);
                        cleared += (u32)__popcll(atomicAnd(&a.bm[w0 + t], ~m) & m);
                    }
                cleared = row8_sum(cleared);
                if (sub == 0) {
                    a.rowflag[j] = 0;
                    if (cleared) {
                        // can == 0 everywhere: the need of a universe is its size
                        const u32 before = atomicSub(&a.usize[a.row_univ[j]], cleared);
                        if (before == cleared) atomicSub(&st->n_need, 1u);
                    }
                }
            }
        }
        if (lig == 0) {
            const u32 slot = atomicAdd(&st->npicks, 1u);
            a.picks[slot] = s;
            a.pick_key[slot] = key;
            a.picked[s] = 1u;
        }
    }
}

// set-up 1/2: rows -> {gs, ge} records + universe bitmap (union of
// every set's rows, set_cover.py:302-320); sets -> first row (binary search in
// the set-sorted table); thread 0 -> the scalar state
__global__ void __launch_bounds__(256)
gf_build_kernel(const i32 *__restrict__ row_set, const i32 *__restrict__ row_univ, const u32 *__restrict__ gs,
                const u32 *__restrict__ ge, u32 nrows_cap, const u32 *__restrict__ nrows_dev, u32 nsets, u32 nrank,
                uint2 *__restrict__ frow, unsigned long long *__restrict__ bm, u32 *__restrict__ set_ptr,
                GreedyState *__restrict__ st) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    // deferred rows: the table's size is only known on the device
    const u32 nrows = nrows_dev ? min(*nrows_dev, nrows_cap) : nrows_cap;
    if (t == 0) st->nrank = nrank;
    if (t < nrows) {
        const u32 s = gs[t], e = ge[t];
        frow[t] = make_uint2(s, e);
        const u32 w0 = s >> 6, w1 = (e - 1) >> 6;
        const u64 m0 = ~0ull << (s & 63), m1 = ~0ull >> (63 - ((e - 1) & 63));
        // deep coverage makes most of these ORs redundant: look first (a stale
        // view only costs a redundant atomic)
        for (u32 w = w0; w <= w1; ++w) {
            u64 m = ~0ull;
            if (w == w0) m &= m0;
            if (w == w1) m &= m1;
            if ((bm[w] & m) != m) atomicOr(&bm[w], m);
        }
    }
    // set_ptr[s] = first row of a set >= s.  The rows are sorted by set: the row
    // standing on a boundary fills the entries of the sets between its
    // predecessor's and its own (a binary search per set was 17 dependent loads)
    if (t < nrows) {
        const u32 cur = (u32)row_set[t];
        const u32 first = t ? (u32)row_set[t - 1] + 1u : 0u;
        for (u32 q = first; q <= cur && q <= nsets; ++q) set_ptr[q] = t;
    }
    if (t <= nsets) {   // sets after the last row's set
        const u32 last = nrows ? (u32)row_set[nrows - 1] + 1u : 0u;
        if (t >= last) set_ptr[t] = nrows;
    }
}

// set-up 2/2: |U_u| per universe (one workgroup each) = what is left to cover
// when every universe has p == 1; counts the universes that need anything
__global__ void __launch_bounds__(256)
gf_universe_kernel(const unsigned long long *bm, const u32 *__restrict__ genome_off, u32 *__restrict__ usize,
                   GreedyState *__restrict__ st, const u32 *__restrict__ info) {
    __shared__ u32 part[4];
    const u32 u = blockIdx.x;
    // deferred rows: a scan that overflowed its work list or a bucket, or rows
    // too long for the 5-word path, stops the solver before the first round
    // (done = 3; the host redoes the group through the synchronous calls)
    if (info && u == 0 && threadIdx.x == 0 && (info[1] != 0 || info[9] > info[12] || info[5] > 257u)) st->done = 3;
    const u32 s = genome_off[u], e = genome_off[u + 1];
    u32 c = 0;
    if (e > s) {
        const u32 w0 = s >> 6, w1 = (e - 1) >> 6;
        for (u32 w = w0 + threadIdx.x; w <= w1; w += blockDim.x) {
            u64 m = ~0ull;
            if (w == w0) m &= ~0ull << (s & 63);
            if (w == w1) m &= ~0ull >> (63 - ((e - 1) & 63));
            c += (u32)__popcll(bm[w] & m);
        }
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 n = part[0] + part[1] + part[2] + part[3];
        usize[u] = n;
        if (n) atomicAdd(&st->n_need, 1u);
    }
}
