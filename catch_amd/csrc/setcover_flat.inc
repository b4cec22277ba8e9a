// Row-parallel ("flat") form of the frontier solver (included by setcover.hip)
// for LARGE instances: the same rounds, the same claims at bitmap-word
// granularity, the same picks as setcover_batched.inc -- but the kernels walk
// ROW records, one lane per row, instead of giving every set to a group of
// lanes.
//
// Why.  With a group of lanes per set a launch is as slow as its unluckiest
// wavefront: sets have 1 to thousands of rows, every set is a chain of
// dependent round trips (set record -> row records -> bitmap words -> owner
// words), and rocprofv3 showed 7 of 32 wave slots per CU occupied on average
// (S4's largest group: 3.96 M sets, 272 M rows, 65 ms in the rounds, the vector
// L1 72 % busy and the VALU 20 %).  And in set order consecutive rows sit in
// different genomes, so every row touches its own 128-byte line of the bitmap
// and of the owner array and nothing is reused before it leaves the L2:
// ~one line fetched per row visit (S4: ~300 GB per step through 4 MB L2s).
//
// Here:
//  * Row ORDER is (tile of the coordinate space, set, start).  Tiles are
//    2^shift bases (at most 8 Mbases: 1 MB of bitmap + 1 MB of owner words,
//    and 16-32 tiles so that every XCD gets two or more); the rows
//    are partitioned by tile in ONE stable pass that forms the record on the
//    way (tile | length | set | word flags in the 64-bit key, the start in the
//    32-bit value); the workgroups of XCD x (blockIdx % 8) sweep the
//    tiles x, x + 8, ... together, so a tile's bitmap and owner words stay in
//    that XCD's L2 while its rows stream past.  Inside a tile rows stay sorted
//    by set: a set's gain is a segmented sum inside the wavefront plus one
//    atomicAdd per run, and the per-set arrays are swept front to back.
//  * Only ALIVE rows are kept: the count launch of every round writes the rows
//    that still hold uncovered elements -- with their new word flags -- densely
//    into the other record buffer (a range per workgroup step, handed out by
//    one atomic per tile counter), so the claim / check / apply launches and
//    the next count stream exactly the alive rows.  (Without it the late
//    rounds of a tile-ordered table cost as much as the early ones: dead and
//    alive rows are interleaved.)
//
//   gr_count   uncovered elements per row -> acc[s] += ..., alive rows out
//   gr_claim   rows of sets of the current rank with acc[s] > 0: raise
//              owner[word] to key(s) = (acc[s], ~s).  Who loses is settled right
//              here: a row that finds (or is handed back by its atomicMax) a
//              larger key marks its own set, a row that raises a word marks the
//              set whose key it displaced -- at the end of the launch exactly the
//              sets that hold every word they claimed are unmarked, and no
//              second pass over the rows is needed to check
//   gr_apply   per SET: the claimants that lost nowhere are recorded, and a
//              wavefront clears the bits of each one's rows -- read from the
//              (set-ordered) row table, a few thousand sets per round, instead
//              of streaming all alive rows once more; the rows of an accepted
//              set then count zero and the next gr_count drops them.  Also
//              zeroes the other owner buffer / gain accumulator / counters
//
// Same preconditions as the fused kernels: every universe fully covered
// (p == 1), rows of at most 257 bases (<= 5 bitmap words).
#define GR_THREADS 512                   // (a step of 2,048 rows per tile-counter atomic; rounds per S4 step: 512 x 4 rows per lane 64.7 ms,
                                         //  256 x 4: 67.6, 768 x 4: 67.8, 512 x 2: 69.2, 256 x 8: 72.8, 1024 x 4: 75.6 -- apply at 256 throughout;
                                         //  again with the 8-byte records of round 4: 512 x 4 50.9, 256 x 6 54.2, 384 x 4 59.5, 640 x 4 61.2,
                                         //  512 x 6 62.4, 512 x 8 66.8)
#define GR_WAVES (GR_THREADS / 64)
#define GR_UNR 4                         // 64-row chunks a wavefront has in flight
#define GR_WCH (64 * GR_UNR)             // rows per wavefront step
#define GR_BCH (GR_WAVES * GR_WCH)       // rows per workgroup step

// The record of an alive row: ONE 64-bit word (round 4; 12 bytes until then -- a 64-bit key with the tile, a cached
// count and a 32-bit set id, plus the 32-bit global start).  The rounds are bound by what they stream (count: the
// records in and the survivors out, claim: the records in again; 2.2e9 row visits per S4 step), and the tile is known
// from where a record lies: start inside the tile (25 bits) | length (9) | flags (5; bit t: word t of the row holds
// uncovered bits) | set (25 bits).  36 -> 24 bytes per row visit.  The cached count went with it (it saved gathers
// that hit the L2 anyway: 17.6 vs 17.3 ms per step with and without, DESIGN.md section 4): every alive row is counted
// again every round.  Instances of more than 2^25 sets take the set-parallel kernels.
#define GR_SET_BITS 25
#define GR_MAX_SETS (1u << GR_SET_BITS)
#define GR_KEY_SET(k) ((u32)(k) & (GR_MAX_SETS - 1u))
#define GR_KEY_FLAGS(k) ((u32)((k) >> GR_SET_BITS) & 0x1fu)
#define GR_KEY_LEN(k) ((u32)((k) >> (GR_SET_BITS + 5)) & 0x1ffu)
#define GR_KEY_LOC(k) ((u32)((k) >> (GR_SET_BITS + 14)))
#define GR_KEY_NOFLAGS(k) ((k) & ~(0x1full << GR_SET_BITS))
#define GR_KEY_MAKE(loc, len, flags, set) (((unsigned long long)(loc) << (GR_SET_BITS + 14)) | ((unsigned long long)(len) << (GR_SET_BITS + 5)) | \
                                           ((unsigned long long)(flags) << GR_SET_BITS) | (unsigned long long)(set))

struct FlatArgs {
    unsigned long long *bm;
    unsigned long long *owner[2];
    unsigned long long *key[2];     // alive rows of round r in buffer r & 1, tile by tile (GR_KEY_*)
    const u32 *tile_ptr;            // first record slot of every tile (ntiles + 1)
    // which tiles the workgroups of XCD x (blockIdx % 8) sweep, in which order: xcd_tile[x * GR_MAXTX + j], j < xcd_ntiles[x].
    // Round 6: dealt by ROWS (largest tile first, to the XCD with the fewest rows so far), not as x, x + 8, ...: a launch
    // ends when the XCD with the most rows is through, and the tiles of a union of unlike groups differ by a factor of ten
    // (S4's union instance: 27.8 M rows on the fullest XCD for 21.8 M on average).  Striped tiles: tile x to XCD x.
    const u32 *xcd_tile, *xcd_ntiles;
    u32 *tile_cnt[2];               // alive rows of every tile in buffer 0 / 1
    // NOTE: always [set_ptr[s], set_end[s]) -- with direct rows set_ptr[s + 1] is NOT the end of set s (gaps, no sentinel)
    const u32 *set_ptr, *set_end;   // the row table in set order (as built by the scan): rows of set s =
    const u32 *row_gs, *row_ge;     //   [set_ptr[s], set_end[s]), their ranges and universes (SoA rows: set_end = set_ptr + 1)
    const i32 *row_univ;
    const uint4 *rows4;             // direct rows (catchhip_rows::rows4): {start, end, universe, bucket} records instead of
                                    //   the three arrays; row indices are slots, a set's rows lie at the front of its bucket
    const u32 *rank;
    u32 *usize;
    u32 *acc[2];                    // gains, accumulated by gr_count of round r in acc[r & 1]
    u32 *claimed, *lost;            // round + 1 when the set claimed / lost a word in that round
    u32 *picked, *picks;
    u32 *alive[2];                  // full coverage, one device: the sets with a gain that were not accepted, listed by the apply
                                    //   launch of round r in alive[r & 1]: the next apply launch sweeps those only.  A SEGMENT per
                                    //   workgroup (alive_seg slots from b * alive_seg, alive_cnt[r & 1][b] filled): workgroup b
                                    //   re-reads what it wrote itself, nothing is appended through a shared counter (one atomic
                                    //   per wavefront on ONE address was 62 k atomics = 0.7 ms per launch on S4's largest group)
    u32 *alive_cnt[2];
    u32 alive_seg;
    unsigned long long *pick_key;
    unsigned long long *blkcnt;     // per workgroup: {row records streamed, rows counted again, bitmap words read, flagged words written}
    GreedyState *st;
    // changed[b] (statistics only, null unless CATCHHIP_FLAT_COUNT_DIRTY): one bit per bitmap word, set by the
    // apply launch of a round of parity b when it clears bits of the word; the count launch of the next round
    // counts the rows that hold such a word -- SURVEY 8(d)'s E_dirty -- beside the rows it counts (all alive ones)
    u32 *changed[2];
    u32 nchg;                       // u32 words of each
    i32 tile_shift;                 // < 0: 8 striped tiles
    // Partial coverage (universe_p < 1; set_cover.py:362-373, 393-433): need[u] = elements of universe u
    // still to be covered (<= 0: finished, its remaining bits are removed), a set's gain is the sum over
    // its universes of min(need[u], count).  uni[b][r] = universe of record r of buffer b | bit 31: its
    // set has a universe in which it holds several rows ("complex": such a set's gain is not a sum of
    // per-row terms and is computed from its rows by gr_fixup).  uT / uM: per universe the two key
    // thresholds of the acceptance rule (gr_usel), see gr_apply.
    u32 partial;
    i32 *need;
    u32 *ufinal;
    unsigned long long *uT, *uM;
    u32 *uni[2];
    const u32 *genome_off;
    const u32 *cset;                // the complex sets; cset[ncset_at] = how many
    u32 ncset_at;
    u32 nsets, nwords, ntiles, nuniv;
    // universes sharded over ranks (setcover_sharded.inc): acc[] has two more slots
    // ([nsets] = universes of THIS rank still in need), gains and lost marks are
    // all-reduced between the launches, the end is decided on the global need
    u32 sharded;
    u32 count0_done;                // acc[0] was filled from the row build's per-set totals: round 0 has no count launch
    u32 pretested;                  // partial coverage, sharded: the universe test of the candidates ran in gr_verdict_kernel
                                    // on every rank and failures travelled with the lost marks -- gr_apply accepts what is left
    unsigned long long inv;         // ~0: bm holds the COVERED positions (starts all zero: nothing to build), 0: the uncovered ones
    // Gain bands (full coverage on one device, no ranks; DESIGN.md section 4 K2).  Gains only fall, so a set's round-0
    // gain bounds its gain for ever: the sets are cut into nbands bands by it (band 0 the highest; band_thr[b] = the
    // lower boundary T_b of band b, the last one's is 1) and every coordinate tile into nbands SUB-TILES, tile * nbands +
    // band -- what tile_ptr, tile_cnt, xcd_tile and ntiles speak of.  A round of level L = st->level[round & 1]
    // streams the sub-tiles of the bands <= L only, and a set claims only with a gain >= T_L: every set that does not
    // claim -- asleep, or counted below T_L -- has a smaller key than every claimant, which is all the acceptance
    // rule needs.  A round without a claimant raises the level.  nbands == 1, T_0 = 1: the rounds as they were.
    //
    // Boundaries per group (rows of a scan with group numbers: a union of independent instances side by side, whose
    // gains differ tenfold -- cut by the instance's largest gain every smaller group would lie below all boundaries,
    // sleep to the last level and then run as without bands).  Group g is cut by ITS largest round-0 gain into the row
    // band_thr[g * nbands + b] = T_b[g]; set_thr[s] = group(s) (null: one row, as above).  The level stays one
    // number for the instance: a round of level L streams the sub-tiles of the bands <= L, and a set claims iff its
    // exact gain reaches T_L[group(s)].  Why that is exact:
    //  * two sets share an uncovered element only inside one group (a probe pairs with its own group's genomes only);
    //  * inside group g every set that does not claim is asleep (round-0 gain, hence gain, below T_L[g]) or counted
    //    below T_L[g]: its gain, hence its key, is smaller than that of every claimant of g;
    //  * so a claimant that holds the largest key on all its words beats every alive set it shares an element with --
    //    all the proof sketch in setcover_batched.inc needs;
    //  * a bitmap word shared by two groups at a group border may make a claimant lose to a set of the other group it
    //    shares no element with: acceptance only becomes more conservative there, as with one row of boundaries;
    //  * late acceptance is harmless -- the set's gain is unchanged until it is accepted -- and the picks are ordered
    //    by their accept-time keys.
    // A group that has emptied its level waits the few rounds the slowest group still needs: one level, so every
    // cross-launch hand-off (level[], wake, fresh, fr_claim) is what it was.
    const u32 *band_thr;
    const u32 *set_thr;
    u32 ngroups;                    // rows of band_thr
    const u8 *band;                 // band of every set (null: one band)
    u32 nbands;
};

// where the set-up kernels (segment flags, the partition by tile) read the (set, start)-ordered rows
struct GrRowSrc {
    const i32 *set, *univ;          // SoA rows
    const u32 *gs, *ge;
    const uint4 *rows4;             // direct rows: {start, end, universe, bucket}; null: SoA
    const u32 *bstart, *mcnt;       //   merged buckets: where a bucket's rows begin and how many there are; null: every slot is a row
    const i32 *bucket_set;          //   set of a bucket; null: the bucket itself
    u32 n;                          // rows (SoA) / slots (direct)
};

// row r of the set-ordered table, in either form (the branch is uniform over the launch)
__device__ __forceinline__ void gr_row_range(const FlatArgs &a, u32 r, u32 &x, u32 &e) {
    if (a.rows4) { const uint2 q = *(const uint2 *)(a.rows4 + r); x = q.x; e = q.y; }
    else { x = a.row_gs[r]; e = a.row_ge[r]; }
}
__device__ __forceinline__ u32 gr_row_univ(const FlatArgs &a, u32 r) { return a.rows4 ? a.rows4[r].z : (u32)a.row_univ[r]; }
__device__ __forceinline__ u32 gr_row_popcount(const FlatArgs &a, u32 r) {
    u32 x, e;
    gr_row_range(a, r, x, e);
    return range_popcount((const u64 *)a.bm, x, e);
}

// What the host knows of a walk when it launches it, as a type: a kernel instance of a form holds only that form's
// paths.  STRIPED: striped (1) or contiguous (0) tiles, BANDED: gain bands (1) or one band (0); -1: as the arguments
// say, decided while the kernel runs (GrAnyForm: the kernels as they were).
template <int STRIPED, int BANDED> struct GrForm {
    static constexpr int striped = STRIPED, banded = BANDED;
    static __device__ __forceinline__ bool is_striped(const int tile_shift) { return STRIPED < 0 ? tile_shift < 0 : STRIPED != 0; }
    static __device__ __forceinline__ bool is_banded(const u32 nbands) { return BANDED < 0 ? nbands > 1 : BANDED != 0; }
};
using GrAnyForm = GrForm<-1, -1>;

// global start of a record of tile t (contiguous tiles: t << shift; striped: 4-kbase stripes dealt round robin)
template <class FORM = GrAnyForm>
__device__ __forceinline__ u32 gr_start(u32 loc, u32 t, int tile_shift) {
    return !FORM::is_striped(tile_shift) ? (t << tile_shift) + loc : ((((loc >> 12) << 3) + t) << 12) | (loc & 4095u);
}
__device__ __forceinline__ u32 gr_loc(u32 x, int tile_shift) {
    return tile_shift >= 0 ? x & ((1u << tile_shift) - 1u) : ((x >> 15) << 12) | (x & 4095u);
}

// the GR_UNR records of this lane in a workgroup step of tile t (dead / out of range: key 0) and their global starts
template <class FORM = GrAnyForm>
__device__ __forceinline__ void load_records(const FlatArgs &a, u32 buf, u32 bbase, u32 end, u32 t,
                                             unsigned long long (&k)[GR_UNR], u32 (&x)[GR_UNR]) {
    const u32 wbase = bbase + (threadIdx.x >> 6) * GR_WCH + (threadIdx.x & 63);
#pragma unroll
    for (int u = 0; u < GR_UNR; ++u) {
        const u32 r = wbase + u * 64;
        k[u] = r < end ? a.key[buf][r] : 0ull;
        x[u] = gr_start<FORM>(GR_KEY_LOC(k[u]), t, a.tile_shift);
    }
}

// Calls f(tile, bbase, end, tile start, k, x) for every workgroup step of GR_BCH
// record slots [bbase, min(bbase + GR_BCH, end)) of buffer `buf` that this
// workgroup takes, with this lane's records of the step in k / x -- loaded one
// step ahead, so that a step's gathers do not wait for its records first.
// The workgroups of XCD x = blockIdx % 8 share the tiles x, x + 8, ...: their
// steps are numbered through (tile after tile) and dealt out round robin, so
// that all workgroups of the XCD sweep the tiles front to back together and
// stay busy when the tiles have shrunk to a few steps each.  Trip counts are
// uniform inside a workgroup.
#define GR_MAXTX 32                      // (sub-)tiles per XCD (256 tiles / 8)
#define GR_BANDS 2                       // gain bands (as far as the tiles allow: FlatSolve::setup) and the ratio of two neighbouring
#define GR_BAND_RATIO 650                //   boundaries in 1/1000.  S4 step, ms: 1 band 74.8-76.6; 2 bands at 0.60 / 0.65 / 0.70: 71.4 / 71.4 /
                                         //   70.1-71.0, at 0.50: 78.5, at 0.75-0.85: 76.9-78.3; 3 at 0.6 / 0.7: 75.7 / 75.9; 4 at 0.7 / 0.8: 80.3 / 73.5;
                                         //   8 at 0.75: 110.8 (every level ends with a round that claims nothing: DESIGN.md section 4 K2)
#define GR_BAND_RATIO_GROUPED 700        // the same for a union cut group by group.  S4 step, ms, three runs each, interleaved: the union with one
                                         //   band 70.6 / 70.5 / 70.3; 2 bands per group at 0.70: 66.9 / 67.0 / 66.7, at 0.65: 70.3 / 70.4 / 70.6 (against
                                         //   71.0 / 70.9 / 71.8), at 0.675 / 0.725: 67.4 / 67.6, at 0.60 (5 steps): 75.9, at 0.75: 71.8; 3 bands at 0.65:
                                         //   74.7 (the large groups, solved alone, at 0.70 beside a union with one band: 70.3 / 70.7 / 70.9 -- they do
                                         //   not care)
#define GR_THR_LDS 1024                 // boundaries per group: the groups whose threshold of the round's level a workgroup keeps in LDS
#define GR_MIN_ROWS ((i64)1 << 18)       // rows from which an instance takes this solver (setcover.hip), and grouped rows their bands
struct GrNoTileHook { __device__ __forceinline__ void operator()(u32, u32) const {} };
// Which sub-tiles a walk takes (gain bands): those of the bands <= level; the sub-tiles of band `wake` (none: ~0)
// are streamed for the first time -- all their records, where the partition put them (buffer 0).
struct GrWalk { u32 level = 0xffffffffu, wake = 0xffffffffu; };
// f(sub-tile, bbase, end, tile start, k, x, fresh): fresh = a step of a band that wakes (uniform over the workgroup)
// on_tile(tile, steps of this XCD in all): called by the whole workgroup before its first step in a tile
// FORM: the walk's form where the caller's instance knows it (GrForm)
template <class FORM = GrAnyForm, class F, class G = GrNoTileHook>
__device__ __forceinline__ void for_each_step(const FlatArgs &a, u32 buf, F f, G on_tile = G(), GrWalk wk = GrWalk()) {
    __shared__ u32 s_first[GR_MAXTX + 1];   // first step number of the XCD's j-th tile
    __shared__ u32 s_tstart[GR_MAXTX], s_tcnt[GR_MAXTX];
    __shared__ u32 s_tile[GR_MAXTX], s_ctile[GR_MAXTX], s_fresh[GR_MAXTX];
    const u32 xcd = blockIdx.x & 7;
    const u32 nbx = (gridDim.x + 7 - xcd) >> 3;        // workgroups on this XCD
    const u32 ntx = min(a.xcd_ntiles[xcd], (u32)GR_MAXTX);
    const bool banded = FORM::is_banded(a.nbands);
    // the tiles' ranges: loaded side by side, kept in LDS for the walk
    if (threadIdx.x < ntx) {
        const u32 tl = a.xcd_tile[xcd * GR_MAXTX + threadIdx.x];
        const u32 band = banded ? tl % a.nbands : 0u;
        const bool fresh = banded && band == wk.wake;
        s_tile[threadIdx.x] = tl;
        s_ctile[threadIdx.x] = banded ? tl / a.nbands : tl;
        s_fresh[threadIdx.x] = fresh ? 1u : 0u;
        s_tstart[threadIdx.x] = a.tile_ptr[tl];
        // (a sleeping band's sub-tiles count as empty: nothing of theirs is read)
        s_tcnt[threadIdx.x] = band > wk.level ? 0u : fresh ? a.tile_ptr[tl + 1] - a.tile_ptr[tl] : a.tile_cnt[buf][tl];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 run = 0;
        for (u32 j = 0; j < ntx; ++j) { s_first[j] = run; run += (s_tcnt[j] + GR_BCH - 1) / GR_BCH; }
        s_first[ntx] = run;
    }
    __syncthreads();
    const u32 total = s_first[ntx];
    u32 j = 0;
    u32 g = blockIdx.x >> 3;
    unsigned long long kc[GR_UNR], kn[GR_UNR];
    u32 xc[GR_UNR], xn[GR_UNR];
    u32 bbase = 0, end = 0;
    if (g < total) {
        while (s_first[j + 1] <= g) ++j;              // steps only move forward
        bbase = s_tstart[j] + (g - s_first[j]) * GR_BCH;
        end = s_tstart[j] + s_tcnt[j];
        load_records<FORM>(a, banded && s_fresh[j] ? 0u : buf, bbase, end, s_ctile[j], kc, xc);
    }
    u32 jprev = 0xffffffffu;
    while (g < total) {
        const u32 jc = j, bc = bbase, ec = end;
        if (jc != jprev) { on_tile(s_tile[jc], total > nbx ? 1u : 0u); jprev = jc; }
        const u32 gn = g + nbx;
        if (gn < total) {
            while (s_first[j + 1] <= gn) ++j;
            bbase = s_tstart[j] + (gn - s_first[j]) * GR_BCH;
            end = s_tstart[j] + s_tcnt[j];
            load_records<FORM>(a, banded && s_fresh[j] ? 0u : buf, bbase, end, s_ctile[j], kn, xn);
        }
        f(s_tile[jc], bc, ec, s_tstart[jc], kc, xc, banded && s_fresh[jc] != 0u);
#pragma unroll
        for (int u = 0; u < GR_UNR; ++u) { kc[u] = kn[u]; xc[u] = xn[u]; }
        g = gn;
    }
    __syncthreads();                                    // the LDS arrays may be rebuilt by a later walk
}

#define GR_USEL_CAP 3072   // words of a universe with uncovered bits that gr_usel lists in LDS (more: it reads them again)
struct __attribute__((aligned(4))) u32x2 { u32 a, b; };

// The uncovered positions of a row of a COVERED bitmap (FlatArgs::inv = ~0) from its words as load_words5 gives them
// with fill ~0 -- a word that was not loaded reads as covered, and an unflagged word of the row that came along with
// its neighbour IS covered in the row's positions, so no word asks for its flag: word 0 is cut at the row's first
// bit, the row's last word at its last bit, what lies past it is masked whole (the masks are made once per row), and
// a word between them costs an OR with zero and its two bit counts.  What is counted is the COVERED
// positions, those outside the row with them (the masks are OR-ed in): 64 in a word that has nothing left, and the
// loaded words are used as they arrive -- a NOT on them is placed by the compiler beside the load, inside the lanes'
// branch, and makes every load wait for its data before the next one is issued.
// Returns the row's uncovered positions; *nf: bit w = word w still holds some (it counted fewer than 64).
// A dead record (key 0, nothing loaded) counts 0 and has no flags.
__device__ __forceinline__ u32 gr_row_uncovered(const unsigned long long (&v)[RP_MAXW], u32 x, u32 len, u32 *nf) {
    const u32 sh = x & 63u, eb = sh + len - 1u, last = eb >> 6;    // the row's last bit, counted from word 0, and its word
    const u64 n0 = ~(~0ull << sh);                                 // below the row's first bit
    const u64 n1 = ~1ull << (eb & 63u);                            // above its last one
    // What lies past the row's last word: load_words5 loads words 0-1 and 2-3 in pairs, so word 1 of a one-word row and
    // word 3 of a three-word row may hold the bitmap of somebody else and are masked whole; word 2 is never loaded past
    // the last word (a flag of word 2 or 3 puts the last word at 2 or beyond), and word 4 only as the last word.
    static_assert(RP_MAXW == 5, "the masks below are written out for five words");
    const bool one = last == 0, upto2 = last <= 2;
    const u64 nw[RP_MAXW] = {n0 | (one ? n1 : 0ull), one ? ~0ull : last > 1 ? 0ull : n1, upto2 ? n1 : 0ull,
                             upto2 ? ~0ull : last > 3 ? 0ull : n1, n1};
    u32 covered = 0, full = 0;
#pragma unroll
    for (u32 w = 0; w < RP_MAXW; ++w) {
        const u64 o = v[w] | nw[w];
        const u32 c = (u32)__popcll(o);
        full |= (c >> 6) << w;                                      // (bit 6 of a count: all 64; taken from the count, so
        covered += c;                                               //  that the word itself need not be kept for it)
    }
    *nf = full ^ ((1u << RP_MAXW) - 1u);
    return 64u * RP_MAXW - covered;
}

// LEAN: the instance of the rounds of a full-coverage solve on one device (covered bitmap, round >= 1, no statistics),
// of the form FORM -- it holds neither round 0, nor the changed-word statistics, nor the other tile form, nor a
// select on FlatArgs::inv.  !LEAN: every path, decided while the kernel runs (FORM = GrAnyForm).
template <bool PARTIAL, bool LEAN = false, class FORM = GrAnyForm>
__global__ void __launch_bounds__(GR_THREADS)
gr_count_kernel(FlatArgs a, u32 round_arg) {
    static_assert(!LEAN || !PARTIAL, "partial coverage keeps an uncovered bitmap");
    __shared__ u32 s_done, s_wcnt[2][GR_WAVES], s_base[2];     // (by step parity: a step's values are read while the next step's are written)
    __shared__ unsigned long long s_rows[4];
    GreedyState *st = a.st;
    if (threadIdx.x == 0) { s_done = st->done; s_rows[0] = s_rows[1] = s_rows[2] = s_rows[3] = 0; }
    __syncthreads();
    if (s_done) return;
    const u32 round = LEAN ? round_arg | 2u : round_arg;  // (LEAN: only its parity and "not 0" are used below)
    const u32 ob = round_arg & 1, ib = round ? ob ^ 1 : 0;    // round 0 counts buffer 0 in place
    u32 *acc = a.acc[ob];
    if (blockIdx.x == 0 && threadIdx.x == 0) st->iters = round_arg + 1;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // LEAN: the rows are counted from the step's ballots, the same in every lane, and the rows counted again are the rows
    u32 cnt_rows = 0, cnt_dirty = 0, cnt_words = 0, cnt_own = 0, step_par = 0;
    // statistics (off in timed runs): words that changed in the previous round's apply launch
    const u32 *chg = !LEAN && a.changed[0] ? a.changed[ob ^ 1] : nullptr;
    // gain bands: the level of this round; a level other than the last round's means that its band wakes now
    GrWalk wk;
    if (FORM::is_banded(a.nbands)) {
        wk.level = st->level[ob];
        if (round && st->level[ob ^ 1] != wk.level) wk.wake = wk.level;
    }
    for_each_step<FORM>(a, ib, [&](u32 t, u32 bbase, u32 end, u32 tstart, unsigned long long (&k)[GR_UNR], u32 (&x)[GR_UNR], bool fresh) {
        // A band that wakes is read from buffer 0.  In an even round that is the buffer being written as well: its
        // records then stay where they are, the dead ones without flags (they claim nothing, and the next count
        // launch drops them), and the step adds its slots to the sub-tile's counter
        const bool inplace = fresh && ob == 0;
        unsigned long long v[GR_UNR][RP_MAXW];
#pragma unroll
        for (int u = 0; u < GR_UNR; ++u) {
            if (LEAN) load_words5(a.bm + (x[u] >> 6), v[u], GR_KEY_FLAGS(k[u]), ~0ull);   // unflagged words: covered for this row
            else if (round && GR_KEY_FLAGS(k[u])) load_words5(a.bm + (x[u] >> 6), v[u], GR_KEY_FLAGS(k[u]));
        }
        u32 nf[GR_UNR], uv[GR_UNR], rc[GR_UNR];
        unsigned long long alive[GR_UNR];
        u32 wtot = 0;
#pragma unroll
        for (int u = 0; u < GR_UNR; ++u) {
            const u32 fl = GR_KEY_FLAGS(k[u]), len = GR_KEY_LEN(k[u]);
            if (LEAN) {
                rc[u] = gr_row_uncovered(v[u], x[u], len, &nf[u]);
                cnt_words += (u32)__popc(fl);
                cnt_own += (u32)__popc(nf[u]);
                alive[u] = __ballot(rc[u] != 0);                // (a row holds uncovered positions iff some word of it does)
                cnt_rows += (u32)__popcll(__ballot(fl != 0));
                wtot += (u32)__popcll(alive[u]);
                continue;
            }
            const u32 e = x[u] + len;
            const u32 w0 = x[u] >> 6, nwd = fl ? ((e - 1) >> 6) - w0 + 1 : 1;
            u32 cnt = 0;
            nf[u] = 0;
            if (fl) {
                cnt_rows++;
                if (round == 0) {
                    // nothing is covered yet and the universe is the union of the rows
                    cnt = len;
                    nf[u] = fl;
                } else {
                    if (chg) {   // SURVEY 8(d)'s E_dirty: rows that hold a word the last picks changed, and their words
                        const u32x2 q = *(const u32x2 *)(chg + (w0 >> 5));
                        const unsigned long long two = (unsigned long long)q.a | ((unsigned long long)q.b << 32);
                        if ((u32)(two >> (w0 & 31u)) & fl) { cnt_dirty++; cnt_words += (u32)__popc(fl); }
                    } else { cnt_dirty++; cnt_words += (u32)__popc(fl); }      // (rows counted again: every alive one)
                    const u64 m0 = ~0ull << (x[u] & 63), m1 = ~0ull >> (63 - ((e - 1) & 63));
#pragma unroll
                    for (u32 w = 0; w < RP_MAXW; ++w) {
                        u64 m = ~0ull;
                        if (w == 0) m &= m0;
                        if (w == nwd - 1) m &= m1;
                        // the row's positions that are still uncovered (unflagged words were not loaded: covered for this row)
                        const u64 um = (w < nwd && ((fl >> w) & 1u)) ? ((v[u][w] ^ a.inv) & m) : 0ull;
                        cnt += (u32)__popcll(um);
                        nf[u] |= um ? (1u << w) : 0u;
                    }
                }
            }
            cnt_own += (u32)__popc(nf[u]);     // owner words this round's claim launch looks at
            if (PARTIAL) {
                // the row's term of its set's gain: min(need of its universe, count) -- exact when the set
                // has one row per universe; rows of complex sets contribute through gr_fixup
                const u32 r = bbase + wave * GR_WCH + lane + u * 64;
                uv[u] = (fl && r < end) ? a.uni[ib][r] : 0u;
                if (fl) {
                    if (uv[u] >> 31) cnt = 0;
                    else { const i32 nd = a.need[uv[u]]; cnt = nd > 0 ? min(cnt, (u32)nd) : 0u; }
                }
            }
            rc[u] = cnt;
            alive[u] = __ballot(nf[u] != 0);
            wtot += (u32)__popcll(alive[u]);
        }
        // alive rows -> the other buffer, densely: one range per workgroup step, handed out by a RETURNING atomic on
        // the tile's counter.  Round 6: it is issued as soon as the step's survivors are counted and its answer is
        // only waited for after the gains' segmented sums below (the whole workgroup used to idle for the round trip
        // between two barriers, 65 times per workgroup and launch on S4's largest group); the LDS cells go by step
        // parity, which spares the third barrier of a step.
        const u32 sp = step_par;
        step_par ^= 1u;
        u32 base_got = 0;
        if (round != 0) {
            if (lane == 0) s_wcnt[sp][wave] = wtot;
            __syncthreads();
            if (threadIdx.x == 0) {
                u32 tot = 0;
                for (int w = 0; w < GR_WAVES; ++w) tot += s_wcnt[sp][w];
                if (inplace) tot = min((u32)GR_BCH, end - bbase);
                base_got = tot ? atomicAdd(&a.tile_cnt[ob][t], tot) : 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < GR_UNR; ++u) {
            // gain of a set = sum over its rows: runs of equal set ids (dead lanes: keys that join no run)
            bool tail;
            const u32 fl = GR_KEY_FLAGS(k[u]);
            const u32 s = fl ? GR_KEY_SET(k[u]) : 0xffffffffu - lane;
            const u32 tot = wave_segsum(rc[u], s, &tail);
            if (tail && tot) atomicAdd(&acc[s], tot);
        }
        if (round == 0) return;     // every row is alive and stays where it is
        if (threadIdx.x == 0) s_base[sp] = base_got;
        __syncthreads();
        u32 o = tstart + s_base[sp];
        for (u32 w = 0; w < wave; ++w) o += s_wcnt[sp][w];
        if (inplace) {
#pragma unroll
            for (int u = 0; u < GR_UNR; ++u) {
                const u32 r = bbase + wave * GR_WCH + lane + u * 64;
                if (r < end) a.key[0][r] = GR_KEY_NOFLAGS(k[u]) | ((unsigned long long)nf[u] << GR_SET_BITS);
            }
            return;
        }
#pragma unroll
        for (int u = 0; u < GR_UNR; ++u) {
            if (nf[u]) {
                const u32 pos = o + (u32)__popcll(alive[u] & ((1ull << lane) - 1ull));
                a.key[ob][pos] = GR_KEY_NOFLAGS(k[u]) | ((unsigned long long)nf[u] << GR_SET_BITS);
                if (PARTIAL) a.uni[ob][pos] = uv[u];
            }
            o += (u32)__popcll(alive[u]);
        }
    }, GrNoTileHook(), wk);
    if (LEAN) { wave_sum_n(cnt_words, cnt_own); cnt_dirty = cnt_rows; }
    else wave_sum_n(cnt_rows, cnt_dirty, cnt_words, cnt_own);
    if (lane == 0) {
        atomicAdd(&s_rows[0], (unsigned long long)cnt_rows);
        atomicAdd(&s_rows[1], (unsigned long long)cnt_dirty);
        atomicAdd(&s_rows[2], (unsigned long long)cnt_words);
        atomicAdd(&s_rows[3], (unsigned long long)cnt_own);
    }
    __syncthreads();
    if (threadIdx.x < 4) a.blkcnt[4 * blockIdx.x + threadIdx.x] += s_rows[threadIdx.x];
    // Some row still holds uncovered elements <=> some universe still needs cover (the universes are
    // the union of the rows): acc[nsets] = "alive rows here" (all-reduced with the gains when the
    // universes are sharded over ranks); the claim launch ends the solve when it is zero.  No
    // per-universe counters: the apply launch then needs neither the rows' universes nor the values its
    // atomics return.
    if (threadIdx.x == 0 && s_rows[3]) atomicOr(&acc[a.nsets], 1u);
}

// BYGROUP: boundaries per group (FlatArgs::set_thr) -- the threshold of a set is fetched where its gain is
template <bool BYGROUP>
__global__ void __launch_bounds__(GR_THREADS)
gr_claim_kernel(FlatArgs a, u32 round) {
    __shared__ u32 s_done, s_claim;
    __shared__ unsigned long long s_cnt[2];
    GreedyState *st = a.st;
    if (threadIdx.x == 0) { s_done = st->done; s_claim = 0; s_cnt[0] = s_cnt[1] = 0; }
    // (round 0 without a count launch: the records and owner words it would have counted are counted here)
    const bool count_here = a.count0_done && round == 0;
    u32 c_rows = 0, c_own = 0;
    __syncthreads();
    if (s_done) return;
    const u32 par = round & 1, cur_rank = st->cur_rank;
    if (blockIdx.x == 0 && threadIdx.x == 0 && st->iters < round + 1) st->iters = round + 1;   // (round 0 may have no count launch)
    if (blockIdx.x == 0 && threadIdx.x == 0) st->nwon = st->npicks;     // (the sets this round accepts are picks[nwon .. npicks): what gr_cover_kernel walks)
    const bool one_rank = st->nrank <= 1;   // no ranks given: nothing to look up per set
    const u32 *acc = a.acc[par];
    unsigned long long *owner = a.owner[par];
    bool any = false;
    // No row anywhere (sharded: on any rank -- acc[] holds the all-reduced values) holds an uncovered
    // element: every universe is covered, finished (all gains are zero then, so nothing is claimed
    // by the workgroups that do not see the flag yet)
    // (gain bands: only at the last level -- before it the sleeping bands may hold such rows, nothing claims, and
    // the apply launch raises the level)
    const u32 level = a.nbands > 1 ? st->level[par] : 0u;
    if (acc[a.nsets] == 0) { if (blockIdx.x == 0 && threadIdx.x == 0 && level + 1 >= a.nbands) st->done = 1; return; }
    const u32 gain_min = a.band_thr[level];     // T_L: what a set must gain to claim in this round (one band: 1)
    // per group: T_L of every group, side by side in LDS (a set's threshold is then one gather, of its group, and an LDS read)
    __shared__ u32 s_thr[BYGROUP ? GR_THR_LDS : 1];
    if (BYGROUP) {
        for (u32 q = threadIdx.x; q < min(a.ngroups, (u32)GR_THR_LDS); q += GR_THREADS) s_thr[q] = a.band_thr[q * a.nbands + level];
        __syncthreads();
    }
    GrWalk wk;
    wk.level = a.nbands > 1 ? level : 0xffffffffu;
    if (a.sharded) {
        // the claimants are decided by the global gains, the same on every rank --
        // also for sets without an alive row here
        for (u32 s = blockIdx.x * GR_THREADS + threadIdx.x; s < a.nsets; s += gridDim.x * GR_THREADS)
            if (acc[s] && a.rank[s] == cur_rank) { any = true; a.claimed[s] = round + 1; }
    }
    for_each_step(a, par, [&](u32, u32 bbase, u32 end, u32, unsigned long long (&k)[GR_UNR], u32 (&x)[GR_UNR], bool) {
        // the set's gain / rank and the owner words depend only on the record:
        // all requested together.  Round 6: the gain (and rank) of a set is fetched by the FIRST lane of its run
        // only and handed to the others by a lane permute -- the launch is bound by the vector memory pipeline's
        // address rate (~1 lane access per CU and cycle, profiles/r06_pmc_rounds_group0.txt), a run is ~20 rows
        // of one set in a tile, and a gather costs what its ACTIVE lanes cost
        const u32 lane = threadIdx.x & 63;
        u32 g[GR_UNR], rk[GR_UNR], hl[GR_UNR];     // (rk: per group the set's threshold -- bands are not cut under ranks)
        unsigned long long heads[GR_UNR];
        unsigned long long seen[GR_UNR][RP_MAXW];
#pragma unroll
        for (int u = 0; u < GR_UNR; ++u) {
            const u32 s = GR_KEY_SET(k[u]);
            const u32 s_prev = __shfl_up(s, 1, WAVE);
            const bool run_head = lane == 0 || s_prev != s;      // (every record of the buffer is alive; slots past the end: set 0, no flags)
            heads[u] = __ballot(run_head);
            hl[u] = 63u - (u32)__clzll(heads[u] & (~0ull >> (63 - lane)));   // first lane of this lane's run
            g[u] = 0; rk[u] = 0;
            if (run_head) {
                g[u] = acc[s];
                if (BYGROUP) { const u32 q = a.set_thr[s]; rk[u] = q < GR_THR_LDS ? s_thr[q] : a.band_thr[q * a.nbands + level]; }
                else rk[u] = one_rank ? 0u : a.rank[s];
            }
            if (GR_KEY_FLAGS(k[u]))
                load_words5(owner + (x[u] >> 6), seen[u], GR_KEY_FLAGS(k[u]));   // owner has slack words; a stale view only costs an atomic
        }
        // Three passes over the step's rows (round 6).  The raises RETURN the word's previous owner, and a lane that
        // looks at one before it issues the next waits a full round trip to the L2 per raise: up to 20 of them in a
        // row per wavefront step (4 chunks x 5 words), 1.3 of the 2.5 ms of the first claim launch on S4's largest
        // group (the replayed loads of the same launch take 1.2 ms, tools/pmc_rounds.sh).  So:
        // every raise of the step is issued first, the answers are looked at afterwards.
        u32 gg[GR_UNR];
        bool claims[GR_UNR], set_claims[GR_UNR];
#pragma unroll
        for (int u = 0; u < GR_UNR; ++u) {
            // (an alive row belongs to a set that was not chosen: the rows of an
            // accepted set count zero and were dropped by gr_count)
            const u32 fl = GR_KEY_FLAGS(k[u]);
            if (count_here && fl) { ++c_rows; c_own += (u32)__popc(fl); }
            gg[u] = __shfl(g[u], (int)hl[u], WAVE);
            const u32 rr = BYGROUP ? cur_rank : one_rank ? 0u : __shfl(rk[u], (int)hl[u], WAVE);
            // (decided per set, so the lanes of a run agree; the first lane of a run
            // stores the marks for all of them)
            // (a band that woke in place leaves dead records, without flags, among its alive ones: such a record may
            // be the first of its set's run, so what the run's first lane stores goes by the set, not by its own record)
            // (per group: the run's first lane compared the gain with its set's threshold -- its bit of the ballot)
            const bool reaches = BYGROUP ? ((__ballot(g[u] >= rk[u]) >> hl[u]) & 1ull) != 0 : gg[u] >= gain_min;
            set_claims[u] = reaches && rr == cur_rank;
            claims[u] = fl && set_claims[u];
        }
#pragma unroll
        for (int u = 0; u < GR_UNR; ++u) {
            if (claims[u]) {
                const u32 fl = GR_KEY_FLAGS(k[u]), s = GR_KEY_SET(k[u]);
                const unsigned long long key = ((unsigned long long)gg[u] << ID_BITS) | (unsigned long long)(ID_MASK - s);
                const u32 w0 = x[u] >> 6;
#pragma unroll
                for (u32 w = 0; w < RP_MAXW; ++w) {
                    // owner words only grow during a launch, so a larger key seen (even in a stale view) is final for
                    // this set; an equal one is another row of the same set
                    if ((fl & (1u << w)) && seen[u][w] < key) {
                        seen[u][w] = atomicMax(&owner[w0 + w], key);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < GR_UNR; ++u) {
            const u32 fl = GR_KEY_FLAGS(k[u]), s = GR_KEY_SET(k[u]);
            bool lost = false;
            if (claims[u]) {
                any = true;
                const unsigned long long key = ((unsigned long long)gg[u] << ID_BITS) | (unsigned long long)(ID_MASK - s);
#pragma unroll
                for (u32 w = 0; w < RP_MAXW; ++w) {
                    if (!(fl & (1u << w))) continue;
                    const unsigned long long other = seen[u][w];
                    if (other > key) lost = true;
                    else if (other && other < key) a.lost[ID_MASK - (u32)other] = round + 1;   // displaced (other < key: this row raised the word)
                }
            }
            // one store per run that lost somewhere, by its first lane (every losing ROW stored until round 6:
            // ~0.9 scattered stores per row visit in the early rounds)
            const unsigned long long lb = __ballot(lost);
            const unsigned long long after = heads[u] & ~((2ull << lane) - 1ull);           // run heads beyond this lane (lane 63: none)
            const unsigned long long upto = after ? ((1ull << (__ffsll((long long)after) - 1)) - 1ull) : ~0ull;
            const bool head = ((heads[u] >> lane) & 1ull) != 0;
            if (head && set_claims[u]) {
                if (lb & upto & ~((1ull << lane) - 1ull)) a.lost[s] = round + 1;
                // (without ranks a set claims iff its gain is not zero: gr_apply looks at the gain instead of a mark)
                if (!one_rank || a.sharded) a.claimed[s] = round + 1;
            }
        }
    }, GrNoTileHook(), wk);
    if (any) s_claim = 1;
    if (count_here) {
        wave_sum_n(c_rows, c_own);
        if ((threadIdx.x & 63) == 0) { atomicAdd(&s_cnt[0], (unsigned long long)c_rows); atomicAdd(&s_cnt[1], (unsigned long long)c_own); }
    }
    __syncthreads();
    if (count_here && threadIdx.x == 0) { a.blkcnt[4 * blockIdx.x] += s_cnt[0]; a.blkcnt[4 * blockIdx.x + 3] += s_cnt[1]; }
    if (threadIdx.x == 0 && s_claim) st->fr_claim[par] = 1;
}

#define GA_SWEEP_MAX 2048  // sets of a workgroup's segment swept per piece (the LDS list of the accepted ones)
#define GA_THREADS 256   // (the apply launch walks sets, not records: 256 threads, as measured -- 7.6 vs 10.3 ms per S4 step with 512)
// PARTIAL (universe_p < 1).  With min(need[u], .) a pick lowers the gain of EVERY set of its universe
// once the need binds, and a universe that reaches its need drops out altogether: holding the largest key
// on its words no longer makes a set safe to accept.  The rule (CPU model: tests/sim_partial_rounds.py,
// which reproduces the oracle's picks in its order):  a word-owning set c is accepted iff for every
// universe u in which it still covers something   key(c) >= uT[u]  or  key(c) >= uM[u]   with
//   uM[u] = the largest owner key on a word of u that holds uncovered bits, and
//   uT[u] = the smallest owner key k of u such that the uncovered bits of u in words owned by keys > k
//           number at most need[u] - smax   (smax bounds what a set covers in one universe).
// Everything picked before c's turn has a larger key and covers only bits in words owned by larger keys,
// so under uT the need of u stays at least c's count until c is the maximum (its gain is what it is now,
// and u is not finished before), and under uM nothing in u is covered before c at all.  The set with the
// largest key of all passes by uM everywhere, so every round makes a pick.
// (Round 6 measured one threshold per LEVEL of what the candidate still covers in u -- bounds 8, 16, ..., smax -- on S4
// at -c 0.9: exact, 1,316 -> 1,205 rounds, but six thresholds per universe in gr_usel and 450 instead of 379 ms per
// solve.  One threshold, bound smax, is what is built.)
// the universe test of candidate sa over the rows [r0, r1) of this device, rows first, first + stride, ...: per
// (set, universe) segment -- the first row of a segment sums it
__device__ __forceinline__ bool gr_passes(const FlatArgs &a, const u32 *acc, u32 sa, u32 r0, u32 r1, u32 first, u32 stride) {
    const unsigned long long key = ((unsigned long long)acc[sa] << ID_BITS) | (unsigned long long)(ID_MASK - sa);
    bool ok = true;
    for (u32 r = r0 + first; r < r1; r += stride) {
        const u32 u = gr_row_univ(a, r);
        if (r > r0 && gr_row_univ(a, r - 1) == u) continue;
        u32 c = 0;
        for (u32 j = r; j < r1 && gr_row_univ(a, j) == u; ++j) c += gr_row_popcount(a, j);
        if (c && !(key >= a.uT[u] || key >= a.uM[u])) ok = false;
    }
    return ok;
}

// Partial coverage with the universes sharded over ranks: a candidate (claimed, lost nowhere) must pass the universe
// test in EVERY universe it still covers something in, and those live on several ranks -- each rank tests its own
// and marks a failing candidate lost; the marks travel once more (the lost exchange) before gr_apply, which then
// accepts every claimant that is not marked (a.pretested).  One wavefront per candidate.
__global__ void __launch_bounds__(GA_THREADS)
gr_verdict_kernel(FlatArgs a, u32 round) {
    if (a.st->done) return;
    const u32 *acc = a.acc[round & 1];
    const u32 lane = threadIdx.x & 63, tag = round + 1;
    const u32 wave = (blockIdx.x * GA_THREADS + threadIdx.x) >> 6, nwaves = (gridDim.x * GA_THREADS) >> 6;
    for (u32 base = wave * 64; base < a.nsets; base += nwaves * 64) {
        const u32 s = base + lane;
        const bool cand = s < a.nsets && a.claimed[s] == tag && a.lost[s] != tag;
        unsigned long long todo = __ballot(cand);
        while (todo) {
            const u32 sa = base + (u32)__ffsll((long long)todo) - 1u;
            todo &= todo - 1ull;
            const u32 r0 = a.set_ptr[sa], r1 = a.set_end[sa];
            if (__ballot(!gr_passes(a, acc, sa, r0, r1, lane, 64u)) && lane == 0) a.lost[sa] = tag;
        }
    }
}

template <bool PARTIAL, bool BYGROUP = false>
__global__ void __launch_bounds__(GA_THREADS)
gr_apply_kernel(FlatArgs a, u32 round) {
    __shared__ u32 s_done;
    GreedyState *st = a.st;
    if (threadIdx.x == 0) s_done = st->done;
    __syncthreads();
    if (s_done) return;
    const u32 par = round & 1;
    const u32 *acc = a.acc[par];
    const u32 gtid = blockIdx.x * GA_THREADS + threadIdx.x, gsize = gridDim.x * GA_THREADS;
    // the other owner buffer, gain accumulator and tile counters serve the next round
    // (full coverage on one device, from round 1 on: only the sets the previous apply launch listed can hold a gain --
    // theirs are the only entries of the other accumulator to clear, and theirs the only marks to look at)
    const bool listed = !PARTIAL && a.alive[0] != nullptr;
    const u32 *in_list = (listed && round > 0) ? a.alive[par ^ 1] : nullptr;
    for (u32 i = gtid; i < a.nwords; i += gsize) a.owner[par ^ 1][i] = 0ull;
    if (!in_list) for (u32 i = gtid; i < a.nsets + 2; i += gsize) a.acc[par ^ 1][i] = 0u;
    else if (gtid < 2) a.acc[par ^ 1][a.nsets + gtid] = 0u;
    for (u32 i = gtid; i < a.ntiles; i += gsize) a.tile_cnt[par ^ 1][i] = 0u;
    if (a.changed[0]) for (u32 i = gtid; i < a.nchg; i += gsize) a.changed[par ^ 1][i] = 0u;   // (statistics; marked by the next round's apply)
    // gain bands: the level of this round (the next round's is written below, into the other cell: no workgroup of
    // this launch reads what thread 0 writes)
    const u32 level = a.nbands > 1 ? st->level[par] : 0u;
    const u32 gain_min = a.band_thr[level];
    if (gtid == 0) {
        const u32 claimed = st->fr_claim[par];
        st->fr_claim[par ^ 1] = 0;
        st->fr_claim[par] = 0;
        u32 next_level = level;
        // nothing claimed although rows with uncovered elements exist (or the claim launch
        // would have set the finished flag)
        if (claimed == 0) {
            if (level + 1 < a.nbands) next_level = level + 1;     // no awake set gains T_L any more: the next band wakes
            else {
                // no set of this rank covers anything still needed: next rank
                const u32 nr = st->cur_rank + 1;
                st->cur_rank = nr;
                if (nr >= st->nrank) st->done = 2;
            }
        }
        if (a.nbands > 1) st->level[par ^ 1] = next_level;
    }
    const u32 lane = threadIdx.x & 63;
    const bool gain_claims = st->nrank <= 1 && !a.sharded;   // (see gr_claim_kernel: no claim marks then)
    if (!PARTIAL) {
        // Full coverage (round 6): this launch only FINDS the accepted sets -- a streaming sweep over the per-set
        // marks, a wavefront per 64 sets, no workgroup barriers -- records them as picks and lists them;
        // gr_cover_kernel then gives every listed set a workgroup.  (Until round 5 the workgroup that found accepted
        // sets walked their rows itself, one set after the other between barriers: 100-165 us per launch on S4's
        // largest group whatever the round held -- the last twelve rounds of its solve were this launch.)
        // workgroup b sweeps its own segment: sets [b * seg, (b + 1) * seg) in round 0 (and whenever nothing is listed),
        // afterwards the sets it listed itself in the previous round
        __shared__ u32 s_out, s_nwin, s_slot0;
        __shared__ u32 s_win[GA_SWEEP_MAX], s_wing[GA_SWEEP_MAX];
        const u32 seg = listed ? a.alive_seg : (a.nsets + gridDim.x - 1) / gridDim.x;
        const u32 seg0 = blockIdx.x * seg;
        const u32 nin = in_list ? a.alive_cnt[par ^ 1][blockIdx.x] : (seg0 < a.nsets ? min(seg, a.nsets - seg0) : 0u);
        u32 *out_list = listed ? a.alive[par] + seg0 : nullptr;
        __shared__ u32 s_thr[BYGROUP ? GR_THR_LDS : 1];     // T_L of every group (see gr_claim_kernel)
        if (BYGROUP)
            for (u32 q = threadIdx.x; q < min(a.ngroups, (u32)GR_THR_LDS); q += GA_THREADS) s_thr[q] = a.band_thr[q * a.nbands + level];
        if (threadIdx.x == 0) { s_out = 0; s_nwin = 0; }
        __syncthreads();
        // The accepted sets of the segment are gathered in LDS and get their places among the picks by ONE atomic per
        // workgroup (a wavefront each was up to 8,000 atomics on one address in the rounds that accept most: 90 us of a
        // launch that otherwise takes 35).  A segment longer than the LDS list is swept in pieces.
        for (u32 piece = 0; piece < nin; piece += GA_SWEEP_MAX) {
            const u32 pend = min(nin, piece + GA_SWEEP_MAX);
            for (u32 base = piece + (threadIdx.x >> 6) * 64; base < pend; base += GA_THREADS) {
                const u32 idx = base + lane;
                const bool valid = idx < pend;
                const u32 s = valid ? (in_list ? in_list[seg0 + idx] : seg0 + idx) : 0u;
                const u32 g = valid ? acc[s] : 0u;
                // (a set claimed iff it gained T_L: a sleeping set's round-0 gain, which round 0 finds here, is below it)
                u32 g_min = gain_min;
                if (BYGROUP) { const u32 q = a.set_thr[s]; g_min = q < GR_THR_LDS ? s_thr[q] : a.band_thr[q * a.nbands + level]; }   // (T_L of the set's own group)
                const bool won = valid && (gain_claims ? g >= g_min : a.claimed[s] == round + 1) && a.lost[s] != round + 1;
                if (in_list && valid) a.acc[par ^ 1][s] = 0u;
                const unsigned long long wb = __ballot(won);
                if (wb) {
                    u32 l0 = 0;
                    if (lane == 0) l0 = atomicAdd(&s_nwin, (u32)__popcll(wb));
                    l0 = __shfl(l0, 0, WAVE);
                    if (won) {
                        const u32 at = l0 + (u32)__popcll(wb & ((1ull << lane) - 1ull));
                        s_win[at] = s; s_wing[at] = g;
                        a.picked[s] = 1u;
                        // (an accepted set's gain is spent: every non-zero entry this launch leaves in this accumulator
                        // belongs to a listed set, so the launch after the next clears them all through its lists)
                        if (listed) a.acc[par][s] = 0u;
                    }
                }
                if (out_list) {
                    // (the segment being read and the one being written are different buffers)
                    // (a set of a sleeping band stays listed: its gain is zero only because nothing counted it)
                    const bool still = valid && !won && (g != 0u || (a.band && a.band[s] > level));
                    const unsigned long long sb = __ballot(still);
                    if (sb) {
                        u32 o0 = 0;
                        if (lane == 0) o0 = atomicAdd(&s_out, (u32)__popcll(sb));
                        o0 = __shfl(o0, 0, WAVE);
                        if (still) out_list[o0 + (u32)__popcll(sb & ((1ull << lane) - 1ull))] = s;
                    }
                }
            }
            __syncthreads();
            const u32 nw = s_nwin;
            if (threadIdx.x == 0 && nw) s_slot0 = atomicAdd(&st->npicks, nw);
            __syncthreads();
            for (u32 q = threadIdx.x; q < nw; q += GA_THREADS) {
                const u32 slot = s_slot0 + q;
                a.picks[slot] = s_win[q];
                a.pick_key[slot] = ((unsigned long long)s_wing[q] << ID_BITS) | (unsigned long long)(ID_MASK - s_win[q]);
            }
            __syncthreads();
            if (threadIdx.x == 0) s_nwin = 0;
            __syncthreads();
        }
        __syncthreads();
        if (listed && threadIdx.x == 0) a.alive_cnt[par][blockIdx.x] = s_out;
        return;
    }
    // Partial coverage: 256 sets per workgroup step; the whole workgroup then walks the rows of each
    // accepted one (a set has up to one row per genome, and a row is a chain of
    // dependent round trips -- bitmap word, atomicAnd: one wavefront per set left a
    // 28-step tail on a 1,769-row set, 130 us per launch)
    __shared__ u32 s_won[GA_THREADS], s_nwon, s_pass;
    for (u32 base = blockIdx.x * GA_THREADS; base < a.nsets; base += gridDim.x * GA_THREADS) {
        const u32 s = base + threadIdx.x;
        const bool won = s < a.nsets && (gain_claims ? acc[s] != 0u : a.claimed[s] == round + 1) && a.lost[s] != round + 1;
        if (threadIdx.x == 0) s_nwon = 0;
        __syncthreads();
        const unsigned long long wb = __ballot(won);
        u32 slot0 = 0, l0 = 0;
        if (lane == 0 && wb) {
            if (!PARTIAL) slot0 = atomicAdd(&st->npicks, (u32)__popcll(wb));
            l0 = atomicAdd(&s_nwon, (u32)__popcll(wb));
        }
        slot0 = __shfl(slot0, 0, WAVE);
        l0 = __shfl(l0, 0, WAVE);
        if (won) {
            const u32 before = (u32)__popcll(wb & ((1ull << lane) - 1ull));
            if (!PARTIAL) {
                a.picks[slot0 + before] = s;
                a.pick_key[slot0 + before] = ((unsigned long long)acc[s] << ID_BITS) | (unsigned long long)(ID_MASK - s);
                a.picked[s] = 1u;
            }
            s_won[l0 + before] = s;
        }
        __syncthreads();
        const u32 nwon = s_nwon;
        // the universe test of a candidate: per (set, universe) segment -- the first row of a segment sums it
        auto passes = [&](u32 sa, u32 r0, u32 r1, u32 first, u32 stride) {
            return a.pretested ? true : gr_passes(a, acc, sa, r0, r1, first, stride);
        };
        auto record_pick = [&](u32 sa) {
            const u32 slot = atomicAdd(&st->npicks, 1u);
            a.picks[slot] = sa;
            a.pick_key[slot] = ((unsigned long long)acc[sa] << ID_BITS) | (unsigned long long)(ID_MASK - sa);
            a.picked[sa] = 1u;
        };
        // the rows of an accepted set leave the universe
        auto cover_rows = [&](u32 r0, u32 r1, u32 first, u32 stride) {
            for (u32 r = r0 + first; r < r1; r += stride) {
                u32 x, e;
                gr_row_range(a, r, x, e);
                const u32 w0 = x >> 6, nwd = ((e - 1) >> 6) - w0 + 1;
                const u64 m0 = ~0ull << (x & 63), m1 = ~0ull >> (63 - ((e - 1) & 63));
                // The accepted sets of a round share no word in which they hold uncovered bits, so a
                // row's own bits are only ever cleared by itself: a plain look at the word tells exactly
                // which of them are still set, and the atomics need not return anything (rows of at
                // most 5 words: all requested before the first use)
                u64 v[RP_MAXW];
#pragma unroll
                for (u32 t = 0; t < RP_MAXW; ++t) v[t] = t < nwd ? a.bm[w0 + t] : 0ull;
                u32 cleared = 0;
#pragma unroll
                for (u32 t = 0; t < RP_MAXW; ++t) {
                    u64 m = ~0ull;
                    if (t == 0) m &= m0;
                    if (t == nwd - 1) m &= m1;
                    if (t < nwd && ((v[t] ^ a.inv) & m)) {
                        if (a.inv) atomicOr(&a.bm[w0 + t], m); else atomicAnd(&a.bm[w0 + t], ~m);
                        if (a.changed[0]) atomicOr(&a.changed[par][(w0 + t) >> 5], 1u << ((w0 + t) & 31u));   // (statistics)
                        if (PARTIAL) cleared += (u32)__popcll(v[t] & m);      // (partial coverage keeps the uncovered positions)
                    }
                }
                if (PARTIAL && cleared) atomicSub(&a.need[gr_row_univ(a, r)], (i32)cleared);
            }
        };
        if (PARTIAL) {
            // Partial coverage: every word-owning set is a candidate and most fail the universe test, so the
            // candidates of up to 256 rows take one wavefront each (four at a time per workgroup) ...
            for (u32 q = threadIdx.x >> 6; q < nwon; q += GA_THREADS / 64) {
                const u32 sa = s_won[q];
                const u32 r0 = a.set_ptr[sa], r1 = a.set_end[sa];
                if (r1 - r0 > 256u) continue;
                if (__ballot(!passes(sa, r0, r1, lane, 64u))) continue;   // stays alive; another round
                if (lane == 0) record_pick(sa);
                cover_rows(r0, r1, lane, 64u);
            }
            __syncthreads();
        }
        // ... and the others (partial coverage: the long ones) the whole workgroup
        for (u32 q = 0; q < nwon; ++q) {
            const u32 sa = s_won[q];
            const u32 r0 = a.set_ptr[sa], r1 = a.set_end[sa];
            if (PARTIAL) {
                if (r1 - r0 <= 256u) continue;
                if (threadIdx.x == 0) s_pass = 1u;
                __syncthreads();
                if (!passes(sa, r0, r1, threadIdx.x, GA_THREADS)) s_pass = 0u;
                __syncthreads();
                const u32 pass = s_pass;
                __syncthreads();          // (s_pass is rewritten for the next candidate)
                if (!pass) continue;      // stays alive; another round
                if (threadIdx.x == 0) record_pick(sa);
            }
            cover_rows(r0, r1, threadIdx.x, GA_THREADS);
        }
        __syncthreads();     // s_won / s_nwon are rewritten by the next step
    }
}

// Full coverage: the rows of the sets gr_apply_kernel<false> listed leave the universe -- a workgroup per accepted set
// (a set has up to one row per genome: 1,769 on S4's largest group), workgroups beyond the list end at once.
__global__ void __launch_bounds__(GA_THREADS)
gr_cover_kernel(FlatArgs a, u32 round) {
    GreedyState *st = a.st;
    if (st->done) return;
    const u32 first = st->nwon, last = st->npicks, par = round & 1;      // the picks of this round
    for (u32 q = first + blockIdx.x; q < last; q += gridDim.x) {
        const u32 sa = a.picks[q];
        const u32 r0 = a.set_ptr[sa], r1 = a.set_end[sa];
        for (u32 r = r0 + threadIdx.x; r < r1; r += GA_THREADS) {
            u32 x, e;
            gr_row_range(a, r, x, e);
            const u32 w0 = x >> 6, nwd = ((e - 1) >> 6) - w0 + 1;
            const u64 m0 = ~0ull << (x & 63), m1 = ~0ull >> (63 - ((e - 1) & 63));
            // The accepted sets of a round share no word in which they hold uncovered bits, so a row's own bits are
            // only ever cleared by itself: a plain look at the word tells exactly which of them are still set, and
            // the atomics need not return anything (rows of at most 5 words: all requested before the first use)
            u64 v[RP_MAXW];
#pragma unroll
            for (u32 t = 0; t < RP_MAXW; ++t) v[t] = t < nwd ? a.bm[w0 + t] : 0ull;
#pragma unroll
            for (u32 t = 0; t < RP_MAXW; ++t) {
                u64 m = ~0ull;
                if (t == 0) m &= m0;
                if (t == nwd - 1) m &= m1;
                if (t < nwd && ((v[t] ^ a.inv) & m)) {
                    if (a.inv) atomicOr(&a.bm[w0 + t], m); else atomicAnd(&a.bm[w0 + t], ~m);
                    if (a.changed[0]) atomicOr(&a.changed[par][(w0 + t) >> 5], 1u << ((w0 + t) & 31u));   // (statistics)
                }
            }
        }
    }
}

// ---- partial coverage: the kernels around the three round launches --------------------------------
// multi-row segments: largest (set, universe) element count -> st->smax, cflag[s] = 1 for a set that
// holds several rows in one universe
__global__ void __launch_bounds__(256)
gr_seg_flag_kernel(GrRowSrc src, u32 *__restrict__ cflag, GreedyState *__restrict__ st) {
    __shared__ u32 s_max[4];
    u32 best = 0;
    const i32 *__restrict__ row_set = src.set, *__restrict__ row_univ = src.univ;
    const u32 *__restrict__ gs = src.gs, *__restrict__ ge = src.ge;
    const u32 nrows = src.n;
    // (grid-stride: one atomic on the shared maximum per workgroup, not per wavefront of rows)
    for (u32 r = blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += gridDim.x * blockDim.x) {
        if (src.rows4) {
            // direct rows: a bucket is a set, and the slot before a row's is a row of its bucket or another bucket's slot
            const uint4 q = src.rows4[r];
            const u32 end = src.mcnt ? src.bstart[q.w] + src.mcnt[q.w] : nrows;
            if (r >= end) continue;                     // a stale record behind the bucket's merged rows
            bool head = r == 0;
            if (!head) { const uint4 pq = src.rows4[r - 1]; head = pq.w != q.w || pq.z != q.z; }
            if (head) {
                u32 tot = 0, j = r;
                for (; j < end; ++j) {
                    const uint4 qj = src.rows4[j];
                    if (qj.w != q.w || qj.z != q.z) break;
                    tot += qj.y - qj.x;
                }
                if (j > r + 1) cflag[src.bucket_set ? (u32)src.bucket_set[q.w] : q.w] = 1u;
                best = tot > best ? tot : best;
            }
            continue;
        }
        if (r == 0 || row_set[r - 1] != row_set[r] || row_univ[r - 1] != row_univ[r]) {
            u32 tot = 0, j = r;
            for (; j < nrows && row_set[j] == row_set[r] && row_univ[j] == row_univ[r]; ++j) tot += ge[j] - gs[j];
            if (j > r + 1) cflag[row_set[r]] = 1u;
            best = tot > best ? tot : best;
        }
    }
    best = wave_max(best);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) best = s_max[i] > best ? s_max[i] : best;
        if (best) atomicMax(&st->smax, best);
    }
}
// list of the flagged sets (pos = exclusive scan of cflag); cset[nsets] = their number
__global__ void __launch_bounds__(256)
gr_cset_kernel(const u32 *__restrict__ cflag, const u32 *__restrict__ pos, u32 nsets, u32 *__restrict__ cset) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nsets && cflag[s]) cset[pos[s]] = s;
    if (s == nsets - 1) cset[nsets] = pos[s] + cflag[s];
}
// need[u] = |U_u| - int(|U_u| - p |U_u|) (set_cover.py:362-373, IEEE double without fused multiply-add)
__global__ void __launch_bounds__(256)
gr_need_init_kernel(const u32 *__restrict__ usize, const double *__restrict__ p, u32 nuniv, i32 *__restrict__ need) {
    const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nuniv) return;
    const double n = (double)usize[u];
    const double prod = __dmul_rn(p[u], n);
    const double diff = __dsub_rn(n, prod);
    long long c = (long long)diff;
    if (c < 0) c = 0;
    if (c > (long long)usize[u]) c = usize[u];
    need[u] = (i32)(usize[u] - (u32)c);
}
// the gain of every complex set from its rows (set order): per universe min(need, sum of its rows' counts)
__global__ void __launch_bounds__(256)
gr_fixup_kernel(FlatArgs a, u32 round) {
    if (a.st->done) return;
    u32 *acc = a.acc[round & 1];
    const u32 ncs = a.cset[a.ncset_at];
    const u32 lane = threadIdx.x & 63;
    for (u32 i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < ncs; i += (gridDim.x * blockDim.x) >> 6) {
        const u32 s = a.cset[i];
        const u32 r0 = a.set_ptr[s], r1 = a.set_end[s];
        u32 tot = 0;
        for (u32 r = r0 + lane; r < r1; r += 64) {
            const u32 u = gr_row_univ(a, r);
            if (r > r0 && gr_row_univ(a, r - 1) == u) continue;
            u32 c = 0;
            for (u32 j = r; j < r1 && gr_row_univ(a, j) == u; ++j) c += gr_row_popcount(a, j);
            const i32 nd = a.need[u];
            if (nd > 0) tot += c < (u32)nd ? c : (u32)nd;
        }
        tot = wave_sum(tot);
        if (lane == 0) acc[s] = a.picked[s] ? 0u : tot;
    }
}
// uT[u], uM[u] from the owner words of this round (one workgroup per universe): a radix select over the
// owner keys of u's words, weighted by the uncovered bits of u they hold, from the most significant byte
__global__ void __launch_bounds__(256)
gr_usel_kernel(FlatArgs a, u32 round) {
    // The words of u that still hold uncovered bits -- a tenth of them on the plateau of a solve -- are listed in
    // LDS by the first pass (owner key, weight); the other passes of the select read the list, not the bitmap and
    // owner words again (round 3: 8 passes over both arrays were 97 of the 476 ms of S4's solves at -c 0.9).
    __shared__ unsigned long long s_hist[256], s_scan[256], s_prefix, s_max[4];
    __shared__ unsigned long long s_k[GR_USEL_CAP];
    __shared__ u32 s_w[GR_USEL_CAP];
    __shared__ long long s_x;
    __shared__ u32 s_n;
    GreedyState *st = a.st;
    if (st->done) return;
    const u32 u = blockIdx.x, tid = threadIdx.x;
    const i32 nd = a.need[u];
    const u32 g0 = a.genome_off[u], g1 = a.genome_off[u + 1];
    if (nd <= 0 || g1 <= g0) {
        if (tid == 0) { a.uT[u] = ~0ull; a.uM[u] = ~0ull; }
        return;
    }
    const unsigned long long *owner = a.owner[round & 1];
    const u32 w0 = g0 >> 6, w1 = (g1 - 1) >> 6;
    const u32 smax = st->smax;
    unsigned long long mx = 0;
    const long long x0 = (long long)nd - (long long)smax;
    if (tid == 0) { s_prefix = 0; s_x = x0; s_n = 0; }
    bool stop = false;
    for (int byte = 7; byte >= 0; --byte) {
        s_hist[tid] = 0;
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        const long long x = s_x;
        const u32 nl = s_n;
        if (byte == 7 || nl > GR_USEL_CAP) {
            for (u32 w = w0 + tid; w <= w1; w += 256) {
                u64 m = ~0ull;
                if (w == w0) m &= ~0ull << (g0 & 63);
                if (w == w1) m &= ~0ull >> (63 - ((g1 - 1) & 63));
                const u32 wt = (u32)__popcll(a.bm[w] & m);
                if (!wt) continue;
                const unsigned long long k = owner[w];
                if (byte == 7) {
                    mx = k > mx ? k : mx;
                    const u32 at = atomicAdd(&s_n, 1u);
                    if (at < GR_USEL_CAP) { s_k[at] = k; s_w[at] = wt; }
                }
                if (x0 >= 0 && (byte == 7 || (k >> (8 * (byte + 1))) == prefix)) atomicAdd(&s_hist[(k >> (8 * byte)) & 0xffu], (unsigned long long)wt);
            }
        } else {
            for (u32 q = tid; q < nl; q += 256) {
                const unsigned long long k = s_k[q];
                if (byte == 7 || (k >> (8 * (byte + 1))) == prefix) atomicAdd(&s_hist[(k >> (8 * byte)) & 0xffu], (unsigned long long)s_w[q]);
            }
        }
        __syncthreads();
        if (x0 < 0) break;                       // (need below the bound: only the top set passes, uM is all that is used)
        // the highest byte value d whose suffix sum (the weight of d and everything above) exceeds x
        unsigned long long T = s_hist[tid];
        for (int off = 1; off < 256; off <<= 1) {
            s_scan[tid] = T;
            __syncthreads();
            if (tid + off < 256) T += s_scan[tid + off];
            __syncthreads();
        }
        const int over = (long long)T > x;         // (suffix sums do not increase with the byte value: a prefix of the threads)
        const int cnt = __syncthreads_count(over);
        if (cnt == 0) { stop = true; break; }     // everything in reach weighs at most x: no threshold
        if ((int)tid == cnt - 1) { s_prefix = (prefix << 8) | (unsigned long long)tid; s_x = x - (long long)(T - s_hist[tid]); }
        __syncthreads();
    }
    if (tid == 0) a.uT[u] = x0 < 0 ? ~0ull : (stop ? 0ull : s_prefix);
    mx = wave_max(mx);
    if ((tid & 63) == 0) s_max[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
        unsigned long long m = s_max[0];
        for (int i = 1; i < 4; ++i) m = s_max[i] > m ? s_max[i] : m;
        a.uM[u] = m;
    }
}
// universes that reached their need drop out: their remaining bits are removed (the rows that held them
// are counted again and die); the last workgroup publishes how many universes are still in need
__global__ void __launch_bounds__(256)
gr_finish_kernel(FlatArgs a, u32 round) {
    GreedyState *st = a.st;
    if (st->done) return;
    const u32 par = round & 1, lane = threadIdx.x & 63;
    const u32 u = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    u32 live = 0;
    if (u < a.nuniv) {
        const i32 nd = a.need[u];
        live = nd > 0 ? 1u : 0u;
        if (nd <= 0 && !a.ufinal[u]) {
            const u32 g0 = a.genome_off[u], g1 = a.genome_off[u + 1];
            if (g1 > g0) {
                const u32 w0 = g0 >> 6, w1 = (g1 - 1) >> 6;
                for (u32 w = w0 + lane; w <= w1; w += 64) {
                    u64 m = ~0ull;
                    if (w == w0) m &= ~0ull << (g0 & 63);
                    if (w == w1) m &= ~0ull >> (63 - ((g1 - 1) & 63));
                    if (a.bm[w] & m) {
                        atomicAnd(&a.bm[w], ~m);
                        if (a.changed[0]) atomicOr(&a.changed[par][w >> 5], 1u << (w & 31u));
                    }
                }
            }
            if (lane == 0) a.ufinal[u] = 1u;
        }
    }
    __shared__ u32 s_live, s_last;
    if (threadIdx.x == 0) s_live = 0;
    __syncthreads();
    if (lane == 0 && live) atomicAdd(&s_live, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_live) atomicAdd(&st->need_live, s_live);
        __threadfence();
        s_last = atomicAdd(&st->ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (s_last && threadIdx.x == 0) {
        __threadfence();
        const u32 n = LD(&st->need_live);
        st->n_need = n;
        if (n == 0 && !a.sharded) st->done = 1;     // (sharded: the claim launch ends the solve on the all-reduced flag)
        st->need_live = 0;
        st->ticket = 0;
    }
}

// Rows -> records in (tile, set, start) order: ONE stable partition of the
// (set, start)-ordered row table by tile.  The record (see GR_KEY_*) is formed
// on the way -- a separate key pass + a generic radix pass read and wrote every
// row once more (S4: 1.9 + 1.2 ms of key and histogram traffic per step).
//
// The rows come in one of two forms (GrRowSrc): the SoA table of a catchhip_rows, or the row build's bucketed
// 16-byte records where they lie (direct rows, catchhip_rows::rows4).  There the index space is the SLOTS of the
// record array: when buckets merged, a bucket's rows sit at the front of its slots and the stale records behind
// them are skipped (slot i of bucket b is a row iff i < bstart[b] + mcnt[b]); when nothing merged every slot is a
// row, mcnt is null and nothing is tested.  Slot order is (set, start) order, so the partition stays stable.
//
// The histogram is [ntiles][blocks] words, tile-major (256 digit rows until round 7, whatever the tile count: with
// S4's 16-30 tiles nine tenths of what was written and scanned were zeros).  The LDS arrays stay 256 wide.
// row (slot) idx: false when there is none; its range, set and universe otherwise
__device__ __forceinline__ bool gr_src_row(const GrRowSrc &src, u32 idx, u32 &x, u32 &e, u32 &sid, u32 &univ) {
    if (idx >= src.n) return false;
    if (src.rows4) {
        const uint4 q = src.rows4[idx];
        if (src.mcnt && idx >= src.bstart[q.w] + src.mcnt[q.w]) return false;
        x = q.x; e = q.y; univ = q.z;
        sid = src.bucket_set ? (u32)src.bucket_set[q.w] : q.w;
        return true;
    }
    x = src.gs[idx]; e = src.ge[idx]; sid = (u32)src.set[idx];
    univ = src.univ ? (u32)src.univ[idx] : 0u;
    return true;
}
#define GT_THREADS 256
#define GT_ROUNDS 16
#define GT_TILE (GT_THREADS * GT_ROUNDS)
// tile_shift < 0: 8 striped tiles (4-kbase stripes dealt round robin)
__device__ __forceinline__ u32 gr_tile_of(u32 x, int tile_shift) { return tile_shift < 0 ? (x >> 12) & 7u : x >> tile_shift; }

// Gain bands.  The boundaries: T_b = ratio^(b + 1) x the largest round-0 gain (ratio in 1/1000), the last one 1.
__global__ void __launch_bounds__(256)
gr_gain_max_kernel(const u32 *__restrict__ gain0, u32 n, GreedyState *__restrict__ st) {
    __shared__ u32 s_max[4];
    u32 best = 0;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) best = max(best, gain0[i]);
    best = wave_max(best);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) best = max(best, s_max[i]);
        if (best) atomicMax(&st->gmax, best);
    }
}
// the group the boundaries of set s go by (catchhip_rows::set_group; a set without a group has no rows: any will do);
// a set with probes in two groups (the flag word behind the sets): every set goes by group 0
__device__ __forceinline__ u32 gr_group_of(const u32 *__restrict__ set_group, u32 nsg, u32 s) {
    if (set_group[nsg] || s >= nsg) return 0u;
    const u32 g = set_group[s];
    return g == 0xffffffffu ? 0u : g;
}
// the same per group: gmax[g] (zeroed) = the largest round-0 gain of group g's sets.  Sets come group after group, so
// every wavefront takes a run of consecutive sets and carries the maximum of the group it is in: an atomic when the
// group changes and one at the end (one per wavefront step was 24,000 atomics on 17 addresses, 0.64 ms, on S4's union;
// 64 sets of several groups in one step: an atomic per lane)
__global__ void __launch_bounds__(256)
gr_group_gain_max_kernel(const u32 *__restrict__ gain0, u32 n, const u32 *__restrict__ set_group, u32 nsg, u32 *__restrict__ gmax) {
    const u32 lane = threadIdx.x & 63;
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const u32 per = ((n + nwaves - 1) / nwaves + 63u) & ~63u;
    const u32 i1 = min(n, (wave + 1) * per);
    u32 cur = 0xffffffffu, best = 0;
    for (u32 i0 = wave * per; i0 < i1; i0 += 64) {
        const u32 i = i0 + lane;
        const u32 v = i < i1 ? gain0[i] : 0u;
        const u32 grp = gr_group_of(set_group, nsg, i < i1 ? i : i1 - 1);
        const u32 grp0 = __shfl(grp, 0, WAVE);
        if (__ballot(grp != grp0) == 0ull) {
            if (grp0 != cur) {
                if (lane == 0 && best) atomicMax(&gmax[cur], best);
                cur = grp0; best = 0;
            }
            best = max(best, wave_max(v));
        } else if (v) atomicMax(&gmax[grp], v);
    }
    if (lane == 0 && best) atomicMax(&gmax[cur], best);
}
__device__ __forceinline__ u32 gr_band_boundary(u32 prev, u32 ratio_pm) {
    return max(1u, (u32)(((unsigned long long)prev * ratio_pm) / 1000ull));
}
// band of every set: the first whose boundary its round-0 gain reaches (sets beyond the gains held: the last).
// gmax[ngroups] / set_group: the groups' largest gains and the sets' groups (one group, set_group null: the instance's
// largest gain) -- thread g < ngroups writes the boundaries of group g, band_thr[g * nbands + b] (a group without
// rows: all 1), and set_thr[s] = the group of set s
__global__ void __launch_bounds__(256)
gr_band_kernel(const u32 *__restrict__ gain0, u32 ng, u32 nsets, GreedyState *__restrict__ st, u32 nbands, u32 ratio_pm,
               u32 *__restrict__ band_thr, u8 *__restrict__ band, const u32 *__restrict__ gmax, u32 ngroups,
               const u32 *__restrict__ set_group, u32 nsg, u32 *__restrict__ set_thr) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < ngroups) {
        u32 t = gmax[s];
        for (u32 b = 0; b + 1 < nbands; ++b) { t = gr_band_boundary(t, ratio_pm); band_thr[s * nbands + b] = t; }
        band_thr[s * nbands + nbands - 1] = 1u;
    }
    if (s == 0) st->band_groups = (set_group && set_group[nsg]) ? 1u : ngroups;
    if (s >= nsets) return;
    const u32 grp = set_group ? gr_group_of(set_group, nsg, s) : 0u;
    const u32 g = s < ng ? gain0[s] : 0u;
    u32 t = gmax[grp], mine = nbands - 1;
    for (u32 b = 0; b + 1 < nbands; ++b) {
        t = gr_band_boundary(t, ratio_pm);
        if (g >= t && mine == nbands - 1) mine = b;
    }
    band[s] = (u8)mine;
    if (set_thr) set_thr[s] = grp;
}

// (band: the band of every set, null with one band -- the partition's digit is the sub-tile, tile * nbands + band)
__global__ void __launch_bounds__(GT_THREADS)
gr_tile_hist_kernel(GrRowSrc src, int tile_shift, u32 ntiles, u32 *__restrict__ hist, u32 nblocks, const u8 *__restrict__ band, u32 nbands) {
    __shared__ u32 h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const u32 base = blockIdx.x * GT_TILE;
    if (band) {
        for (int r = 0; r < GT_ROUNDS; ++r) {
            u32 x = 0u, e = 1u, sid = 0u, univ = 0u;
            if (gr_src_row(src, base + r * GT_THREADS + threadIdx.x, x, e, sid, univ))
                atomicAdd(&h[gr_tile_of(x, tile_shift) * nbands + band[sid]], 1u);
        }
        __syncthreads();
        if (threadIdx.x < ntiles) hist[(size_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
        return;
    }
#pragma unroll 4
    for (int r = 0; r < GT_ROUNDS; ++r) {
        const u32 idx = base + r * GT_THREADS + threadIdx.x;
        if (idx >= src.n) continue;
        if (!src.rows4) atomicAdd(&h[gr_tile_of(src.gs[idx], tile_shift)], 1u);
        else if (!src.mcnt) atomicAdd(&h[gr_tile_of(src.rows4[idx].x, tile_shift)], 1u);
        else {
            const uint4 q = src.rows4[idx];
            if (idx < src.bstart[q.w] + src.mcnt[q.w]) atomicAdd(&h[gr_tile_of(q.x, tile_shift)], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < ntiles) hist[(size_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

__global__ void __launch_bounds__(GT_THREADS)
gr_tile_scatter_kernel(GrRowSrc src, int tile_shift, u32 ntiles, const u32 *__restrict__ hist_scanned, u32 nblocks,
                       unsigned long long *__restrict__ keys, const u32 *__restrict__ cflag, u32 *__restrict__ unis,
                       const u8 *__restrict__ band, u32 nbands) {
    __shared__ u32 wave_cnt[GT_THREADS / 64][256];
    __shared__ u32 base[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 nrows = src.n;
    base[tid] = (u32)tid < ntiles ? hist_scanned[(size_t)tid * nblocks + blockIdx.x] : 0u;
    const u32 tile0 = blockIdx.x * GT_TILE;
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int r = 0; r < GT_ROUNDS; ++r) {
        if (tile0 + (u32)r * GT_THREADS >= nrows) break;   // uniform
        const u32 idx = tile0 + (u32)r * GT_THREADS + tid;
        u32 x = 0u, e = 1u, sid = 0u, univ = 0u;
        const bool valid = gr_src_row(src, idx, x, e, sid, univ);
        const u32 digit = valid ? (band ? gr_tile_of(x, tile_shift) * nbands + band[sid] : gr_tile_of(x, tile_shift)) : 0u;
#pragma unroll
        for (int w = 0; w < GT_THREADS / 64; ++w) wave_cnt[w][tid] = 0;
        __syncthreads();
        // lanes of this wavefront with the same tile (multi-split through ballots)
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        const u32 rank_in_wave = (u32)__popcll(peers & lt_mask);
        if (valid && rank_in_wave == 0) wave_cnt[wave][digit] = (u32)__popcll(peers);
        __syncthreads();
        {
            u32 b = base[tid];
#pragma unroll
            for (int w = 0; w < GT_THREADS / 64; ++w) {
                const u32 c = wave_cnt[w][tid];
                wave_cnt[w][tid] = b;
                b += c;
            }
            base[tid] = b;
        }
        __syncthreads();
        if (valid) {
            const u32 pos = wave_cnt[wave][digit] + rank_in_wave;
            const u32 nwd = ((e - 1) >> 6) - (x >> 6) + 1;
            keys[pos] = GR_KEY_MAKE(gr_loc(x, tile_shift), e - x, (1u << nwd) - 1u, sid);
            if (unis) unis[pos] = univ | (cflag[sid] ? 0x80000000u : 0u);   // partial coverage
        }
        __syncthreads();
    }
}

// first record of every tile (the scanned histogram is tile-major: tile t starts where its first block does),
// and the tiles' sizes
__global__ void __launch_bounds__(256)
gr_tile_ptr_kernel(const u32 *__restrict__ hist_scanned, u32 nblocks, u32 nrows, u32 ntiles, u32 *__restrict__ tile_ptr,
                   u32 *__restrict__ tile_cnt) {
    __shared__ u32 s_ptr[258];
    const u32 t = threadIdx.x;
    for (u32 q = t; q <= ntiles; q += blockDim.x) {
        const u32 v = (q < ntiles && q < 256u && nblocks) ? hist_scanned[(size_t)q * nblocks] : nrows;
        s_ptr[q] = v;
        tile_ptr[q] = v;
    }
    __syncthreads();
    for (u32 q = t; q < ntiles; q += blockDim.x) tile_cnt[q] = s_ptr[q + 1] - s_ptr[q];
}

// the tiles of every XCD (FlatArgs::xcd_tile): by_rows = largest tile first, each to the XCD that holds the fewest rows so far
// (at most GR_MAXTX tiles per XCD; 8 x GR_MAXTX >= ntiles); otherwise tile t to XCD t % 8 as until round 6
__global__ void __launch_bounds__(256)
// Gain bands: ntiles COORDINATE tiles of nbands sub-tiles each (tile_cnt is per sub-tile).  Coordinate tiles are
// dealt, by their rows of all bands, and the lists then name every tile's sub-tiles side by side, band 0 first: they
// stay on one XCD (8 x (GR_MAXTX / nbands) >= ntiles).
gr_tile_assign_kernel(const u32 *__restrict__ tile_cnt, u32 ntiles, u32 nbands, int by_rows, u32 *__restrict__ xcd_tile, u32 *__restrict__ xcd_ntiles) {
    __shared__ u32 s_cnt[256], s_order[256];
    const u32 t = threadIdx.x;
    const u32 max_held = (u32)GR_MAXTX / nbands;
    if (!by_rows) {
        if (t < ntiles)
            for (u32 b = 0; b < nbands; ++b) xcd_tile[(t & 7u) * GR_MAXTX + (t >> 3) * nbands + b] = t * nbands + b;
        if (t < 8) xcd_ntiles[t] = ntiles > t ? ((ntiles - t + 7u) >> 3) * nbands : 0u;
        return;
    }
    {
        u32 c = 0;
        if (t < ntiles) for (u32 b = 0; b < nbands; ++b) c += tile_cnt[t * nbands + b];
        s_cnt[t] = c;
    }
    __syncthreads();
    if (t < ntiles) {
        u32 rk = 0;
        for (u32 q = 0; q < ntiles; ++q) rk += (s_cnt[q] > s_cnt[t] || (s_cnt[q] == s_cnt[t] && q < t)) ? 1u : 0u;
        s_order[rk] = t;
    }
    __syncthreads();
    if (t == 0) {
        unsigned long long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        u32 held[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (u32 r = 0; r < ntiles; ++r) {
            const u32 tl = s_order[r];
            u32 best = 8;
            for (u32 x = 0; x < 8; ++x)
                if (held[x] < max_held && (best == 8 || load[x] < load[best])) best = x;
            xcd_tile[best * GR_MAXTX + held[best]] = tl;
            ++held[best];
            load[best] += s_cnt[tl];
        }
        // ... then moves and swaps between the fullest XCD and the emptiest while that lowers the fuller of the two (the
        // greedy deal of S4's union instance left 23.2 M rows on one XCD and 19.6 M on another for 21.8 M on average)
        for (int it = 0; it < 128; ++it) {
            u32 xa = 0, xb = 0;
            for (u32 x = 1; x < 8; ++x) { if (load[x] > load[xa]) xa = x; if (load[x] < load[xb]) xb = x; }
            if (xa == xb) break;
            const unsigned long long la = load[xa], lb = load[xb];
            unsigned long long best = la;                 // the fuller of the two after the change
            int bi = -1, bj = -1;                         // tile slots: bj < 0 = a move of bi
            for (u32 i = 0; i < held[xa]; ++i) {
                const unsigned long long ca = s_cnt[xcd_tile[xa * GR_MAXTX + i]];
                if (held[xb] < max_held) {
                    const unsigned long long m = la - ca > lb + ca ? la - ca : lb + ca;
                    if (m < best) { best = m; bi = (int)i; bj = -1; }
                }
                for (u32 j = 0; j < held[xb]; ++j) {
                    const unsigned long long cb = s_cnt[xcd_tile[xb * GR_MAXTX + j]];
                    if (cb >= ca) continue;
                    const unsigned long long m = la - ca + cb > lb + ca - cb ? la - ca + cb : lb + ca - cb;
                    if (m < best) { best = m; bi = (int)i; bj = (int)j; }
                }
            }
            if (bi < 0) break;
            const u32 ta = xcd_tile[xa * GR_MAXTX + bi];
            if (bj < 0) {
                xcd_tile[xb * GR_MAXTX + held[xb]++] = ta;
                xcd_tile[xa * GR_MAXTX + bi] = xcd_tile[xa * GR_MAXTX + --held[xa]];
                load[xa] -= s_cnt[ta]; load[xb] += s_cnt[ta];
            } else {
                const u32 tb = xcd_tile[xb * GR_MAXTX + bj];
                xcd_tile[xa * GR_MAXTX + bi] = tb; xcd_tile[xb * GR_MAXTX + bj] = ta;
                load[xa] += s_cnt[tb]; load[xa] -= s_cnt[ta]; load[xb] += s_cnt[ta]; load[xb] -= s_cnt[tb];
            }
        }
        // an XCD sweeps its tiles in ascending tile order (neighbouring tiles' per-set arrays lie side by side)
        for (u32 x = 0; x < 8; ++x) {
            u32 *lst = xcd_tile + x * GR_MAXTX;
            for (u32 i = 1; i < held[x]; ++i) {
                const u32 v = lst[i];
                u32 j = i;
                while (j > 0 && lst[j - 1] > v) { lst[j] = lst[j - 1]; --j; }
                lst[j] = v;
            }
            // coordinate tiles -> their sub-tiles (from the back: slot i * nbands + b lies at or behind slot i)
            if (nbands > 1)
                for (u32 i = held[x]; i-- > 0;) {
                    const u32 ct = lst[i];
                    for (u32 b = nbands; b-- > 0;) lst[i * nbands + b] = ct * nbands + b;
                }
            xcd_ntiles[x] = held[x] * nbands;
        }
    }
}

// universe bitmap = union of every set's rows (set_cover.py:302-320), from the
// tile-ordered records (the tile's words are L2-resident while it is built)
__global__ void __launch_bounds__(GR_THREADS)
gr_bitmap_kernel(FlatArgs a) {
    for_each_step(a, 0, [&](u32, u32 bbase, u32 end, u32, unsigned long long (&k)[GR_UNR], u32 (&x)[GR_UNR], bool) {
#pragma unroll
        for (int u = 0; u < GR_UNR; ++u) {
            if (!GR_KEY_FLAGS(k[u])) continue;
            const u32 e = x[u] + GR_KEY_LEN(k[u]);
            const u32 w0 = x[u] >> 6, w1 = (e - 1) >> 6;
            const u64 m0 = ~0ull << (x[u] & 63), m1 = ~0ull >> (63 - ((e - 1) & 63));
            // deep coverage makes most of these ORs redundant: look first (a stale
            // view only costs a redundant atomic)
            for (u32 w = w0; w <= w1; ++w) {
                u64 m = ~0ull;
                if (w == w0) m &= m0;
                if (w == w1) m &= m1;
                if ((a.bm[w] & m) != m) atomicOr(&a.bm[w], m);
            }
        }
    });
}

// Host side: one zeroed arena, the sort, the set-up launches, three launches per
// round.  FlatSolve holds the state so that the rounds can be driven from
// outside (setcover_sharded.inc puts an all-reduce between the launches).
__global__ void gr_fill_one_kernel(u32 *p, u32 v) { *p = v; }
// direct rows: the slots of every set's rows from its bucket (set_ptr / set_end arrive zeroed: a set without a bucket is empty)
__global__ void __launch_bounds__(256)
gr_set_range_kernel(const u32 *__restrict__ bstart, const u32 *__restrict__ mcnt, const i32 *__restrict__ bucket_set, u32 nb,
                    u32 nsets, u32 *__restrict__ set_ptr, u32 *__restrict__ set_end) {
    const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const u32 s = bucket_set ? (u32)bucket_set[b] : b;
    if (s >= nsets) return;
    set_ptr[s] = bstart[b];
    set_end[s] = bstart[b] + mcnt[b];
}

struct FlatSolve {
    catchhip_ctx *ctx = nullptr;
    DevBuf<u8> arena;
    DevBuf<u64> skey, skey_alt;
    DevBuf<u32> suni, suni_alt;        // partial coverage: the universe of every record
    DevBuf<double> d_p;
    FlatArgs fa;
    unsigned gblocks = 8;
    u32 nsets = 0;
    bool partial = false;

    // h_p: per universe the fraction to cover when some universe may stay partly uncovered, else null
    int setup(catchhip_ctx *c, const catchhip_rows *R, u32 nsets_, const u32 *h_rank, u32 nrank, bool sharded,
              PhaseTimer *tm, const double *h_p = nullptr) {
        ctx = c;
        nsets = nsets_;
        partial = h_p != nullptr;
        hipStream_t s = ctx->stream;
        const u32 nrows = (u32)R->n, nuniv = (u32)R->ngenomes;
        const size_t nwords = (size_t)(R->total / 64 + 2);
        // where the set-up kernels read the rows: the SoA table, or the row build's records in place (direct rows;
        // the validity test of merged buckets only when something merged)
        const bool direct = R->rows4.p != nullptr;
        GrRowSrc src;
        src.set = (const i32 *)R->set_id.p; src.univ = (const i32 *)R->univ.p;
        src.gs = (const u32 *)R->gs.p; src.ge = (const u32 *)R->ge.p;
        src.rows4 = (const uint4 *)R->rows4.p;
        const bool gaps = direct && R->slots != R->n;
        src.bstart = gaps ? (const u32 *)R->bstart.p : nullptr; src.mcnt = gaps ? (const u32 *)R->mcnt.p : nullptr;
        src.bucket_set = direct ? R->bucket_set : nullptr;
        src.n = direct ? (u32)R->slots : nrows;
        // a multiple of 8, at least 8: workgroup b serves the tiles of XCD b % 8
        // workgroups per CU: the walk is persistent (for_each_step deals the steps out), so what is resident at once -- 4 x 8
        // wavefronts per CU -- is enough, and the ~20 short launches at the end of every solve start half as many (K2 rounds of
        // an S4 step one chain at a time: 12 per CU 41.8 ms, 8: 40.5 -- the value until round 6 --, 6: 40.3, 4: 40.1)
        const i64 wg_per_cu = std::max<i64>(1, chip_test_env_int("CATCHHIP_FLAT_WG_PER_CU", 4));
        gblocks = (unsigned)(std::max<i64>(8, std::min<i64>(div_up(nrows, GR_BCH), (i64)ctx->num_cus * wg_per_cu)) + 7) & ~7u;
        // Tiles.  A coordinate space whose bitmap + owner words (0.25 B per base) fit
        // the eight L2s together (<= 64 Mbases: 2 MB per XCD) is cut into 8 STRIPED
        // tiles, 4-kbase stripes dealt round robin: every XCD keeps its eighth
        // resident, the XCDs get equal work, and the rows in flight spread over the
        // whole tile (small contiguous tiles put dozens of concurrent claimants on
        // every owner word: claim 407 us vs check 100 us on 19 M rows).  Larger ones
        // get contiguous tiles of at most 16 Mbases (2 + 2 MB; 8 Mbases until round 3: 64.5 vs 63.1 ms in the
        // rounds of an S4 step), 16-32 of them so that every XCD sweeps several, at most 256 (one radix pass).
        int tile_shift = -1;
        u32 ntiles = 8;
        const int forced_shift = (int)chip_test_env_int("CATCHHIP_FLAT_TILE_SHIFT", -1);
        if (((u64)R->total > ((u64)64 << 20) || forced_shift >= 0) && !chip_test_env("CATCHHIP_FLAT_STRIPED")) {
            // (partial coverage: hundreds of rounds over the tenth of the rows that stays alive, in which what a
            // round moves is the per-set arrays once per tile -- 8 tiles of up to 32 Mbases: 198 -> 159 ms on
            // S4's largest group)
            const int max_shift = partial ? 25 : 24;
            // (round 6, the kernels of rounds 4-6: 16 tiles of 16 Mbases beat 32 of 8 on S4's largest group -- 16.8 vs 17.8 ms
            // in the rounds; 8 of 32 Mbases: 16.9 -- so at least 8 tiles, one per XCD, whatever the coverage; 16 until then)
            // A union of independent groups (rows of a scan with group numbers) gets 16 tiles at least: its tiles differ
            // tenfold in rows, and 30 of them are dealt to 8 XCDs more evenly than 15 (S4's union instance: 24.1 M rows on the
            // fullest XCD with 15 tiles, for 21.8 M on average) -- worth more there than the longer runs of larger tiles.
            const u64 min_tiles = (u64)std::max<i64>(1, chip_test_env_int("CATCHHIP_FLAT_MIN_TILES", R->grouped && !partial ? 16 : 8));
            tile_shift = 16;
            while (tile_shift < max_shift && ((u64)R->total >> (tile_shift + 1)) >= min_tiles) ++tile_shift;
            if (forced_shift >= 0) tile_shift = forced_shift;
            while (((u64)R->total >> tile_shift) >= 256) ++tile_shift;
            ntiles = (u32)((u64)R->total >> tile_shift) + 1;
        }
        // Gain bands: full coverage on one device without ranks, when the rows came with their sets' round-0 gains.
        // As many as asked for (CATCHHIP_FLAT_BANDS; 1: none) and as the tiles allow: every XCD lists at most GR_MAXTX
        // sub-tiles, and the coordinate tiles are dealt to the XCDs whole.
        const bool stats_dirty = chip_test_env("CATCHHIP_FLAT_COUNT_DIRTY") != nullptr;   // E_dirty beside the rows counted (bench: one untimed step)
        u32 nbands = 1;
        if (!partial && !sharded && !h_rank && nrank <= 1 && !stats_dirty && R->gain0_n && nrows) {
            const u32 max_bands = (u32)GR_MAXTX / (u32)div_up((i64)ntiles, 8);
            // (a union of unlike groups is cut group by group, FlatArgs::set_thr, when it is large enough to get here by its
            // own size; a smaller one -- here through CATCHHIP_FLAT_MIN_ROWS -- or one whose rows do not name their sets'
            // groups keeps one band unless asked)
            const i64 grouped_default = (R->set_group_n && (i64)nrows >= GR_MIN_ROWS) ? GR_BANDS : 1;
            const i64 want = R->grouped ? chip_test_env_int("CATCHHIP_FLAT_BANDS_GROUPED", grouped_default) : chip_test_env_int("CATCHHIP_FLAT_BANDS", GR_BANDS);
            nbands = (u32)std::max<i64>(1, std::min<i64>(want, (i64)max_bands));
        }
        // boundaries per group: grouped rows that name the group of every set, more than one band
        const u32 ngroups = (nbands > 1 && R->grouped && R->set_group_n && R->ngroups) ? R->ngroups : 1u;
        const bool by_group = nbands > 1 && R->grouped && R->set_group_n && R->ngroups;
        const u32 band_ratio = (u32)std::max<i64>(1, std::min<i64>(chip_test_env_int("CATCHHIP_FLAT_BAND_RATIO", R->grouped && R->set_group_n ? GR_BAND_RATIO_GROUPED : GR_BAND_RATIO), 999));
        const u32 nsub = ntiles * nbands;                                  // sub-tiles: what the records are partitioned by
        size_t off = 0;
        auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
        const size_t o_bm = take(8 * (nwords + 8)), o_ow0 = take(8 * (nwords + 8)), o_ow1 = take(8 * (nwords + 8)),
                     o_blk = take(32 * (size_t)gblocks), o_st = take(sizeof(GreedyState)),
                     o_picked = take(4 * (size_t)nsets), o_claimed = take(4 * (size_t)nsets),
                     o_lost = take(4 * (size_t)nsets), o_rank = take(4 * (size_t)nsets),
                     o_acc0 = take(4 * ((size_t)nsets + 2)), o_acc1 = take(4 * ((size_t)nsets + 2)),
                     o_tc0 = take(4 * 258), o_tc1 = take(4 * 258), o_gmax = take(by_group ? 4 * (size_t)ngroups : 0);
        const size_t nchg = stats_dirty ? nwords / 32 + 4 : 0;
        const size_t o_chg0 = take(4 * nchg), o_chg1 = take(4 * nchg);
        const size_t o_cflag = take(partial ? 4 * ((size_t)nsets + 1) : 0), o_ufinal = take(partial ? 4 * (size_t)nuniv + 4 : 0);
        // direct rows: set_ptr / set_end are filled from the buckets and must start zeroed (a set without a bucket is empty)
        const size_t o_dsptr = take(direct ? 4 * ((size_t)nsets + 1) : 0), o_send = take(direct ? 4 * ((size_t)nsets + 1) : 0);
        const size_t zero_bytes = off;
        const bool list_alive = !partial && !sharded;
        const u32 alive_seg = (u32)div_up((i64)std::max<u32>(nsets, 1), (i64)gblocks);
        const size_t o_al0 = take(list_alive ? 4 * (size_t)alive_seg * gblocks : 0), o_al1 = take(list_alive ? 4 * (size_t)alive_seg * gblocks : 0),
                     o_alc0 = take(list_alive ? 4 * (size_t)gblocks : 0), o_alc1 = take(list_alive ? 4 * (size_t)gblocks : 0);
        const size_t o_usize = take(4 * (size_t)std::max<u32>(nuniv, 1)), o_picks = take(4 * (size_t)nsets),
                     o_keys = take(8 * (size_t)nsets), o_tptr = take(4 * 258),
                     o_sptr = direct ? o_dsptr : take(4 * ((size_t)nsets + 1)),
                     o_xt = take(4 * 8 * GR_MAXTX), o_xn = take(4 * 8),
                     o_thr = take(4 * std::max<size_t>(GR_MAXTX, (size_t)ngroups * nbands)), o_band = take(nbands > 1 ? (size_t)nsets : 0),
                     o_sthr = take(by_group ? 4 * (size_t)nsets : 0);
        const size_t o_need = take(partial ? 4 * (size_t)nuniv + 4 : 0), o_uT = take(partial ? 8 * (size_t)nuniv + 8 : 0),
                     o_uM = take(partial ? 8 * (size_t)nuniv + 8 : 0), o_cpos = take(partial ? 4 * ((size_t)nsets + 1) : 0),
                     o_cset = take(partial ? 4 * ((size_t)nsets + 2) : 0);
        TRY(arena.alloc(off));
        u8 *A = arena.p;
        if (nsets > GR_MAX_SETS) { chip_set_error("setcover: more than 2^%d sets in the row-parallel solver", GR_SET_BITS); return CATCHHIP_EINVAL; }
        TRY(skey.alloc(std::max<u32>(nrows, 1)));
        TRY(skey_alt.reserve(std::max<u32>(nrows, 1)));
        TRY(chip_pinned_reserve(ctx, sizeof(GreedyState) + 32 * (size_t)gblocks + 12 * (size_t)nsets + 64));
        HIP_TRY(hipMemsetAsync(A, 0, zero_bytes, s));
        {
            GreedyState *h0 = (GreedyState *)ctx->h_pin;   // scalar state: only the rank count is non-zero
            memset(h0, 0, sizeof(GreedyState));
            h0->nrank = nrank;
            HIP_TRY(hipMemcpyAsync(A + o_st, h0, sizeof(GreedyState), hipMemcpyHostToDevice, s));
        }
        if (h_rank) {
            memcpy(ctx->h_big, h_rank, 4 * (size_t)nsets);
            HIP_TRY(hipMemcpyAsync(A + o_rank, ctx->h_big, 4 * (size_t)nsets, hipMemcpyHostToDevice, s));
        }
        fa.partial = partial ? 1u : 0u;
        fa.need = (i32 *)(A + o_need); fa.ufinal = (u32 *)(A + o_ufinal);
        fa.uT = (unsigned long long *)(A + o_uT); fa.uM = (unsigned long long *)(A + o_uM);
        fa.genome_off = (const u32 *)R->genome_off.p;
        fa.cset = (const u32 *)(A + o_cset); fa.ncset_at = nsets;
        fa.uni[0] = fa.uni[1] = nullptr;
        if (partial) {
            TRY(suni.alloc(std::max<u32>(nrows, 1)));
            TRY(suni_alt.reserve(std::max<u32>(nrows, 1)));
            fa.uni[0] = suni.p; fa.uni[1] = suni_alt.p;
            TRY(d_p.alloc(std::max<u32>(nuniv, 1)));
            HIP_TRY(hipMemcpyAsync(d_p.p, h_p, sizeof(double) * nuniv, hipMemcpyHostToDevice, s));
            // sets that hold several rows in one universe, and the largest (set, universe) count
            DevBuf<u32> tmp2;
            hipLaunchKernelGGL(gr_seg_flag_kernel, dim3((unsigned)std::max<i64>(1, std::min<i64>(div_up((i64)src.n, 256), (i64)ctx->num_cus * 16))), dim3(256), 0, s,   // (a shard without rows still takes part)
                               src, (u32 *)(A + o_cflag), (GreedyState *)(A + o_st));
            TRY(chip_exclusive_scan_u32(ctx, (const u32 *)(A + o_cflag), (u32 *)(A + o_cpos), (i64)nsets, tmp2));
            hipLaunchKernelGGL(gr_cset_kernel, dim3((unsigned)div_up((i64)nsets, 256)), dim3(256), 0, s,
                               (const u32 *)(A + o_cflag), (const u32 *)(A + o_cpos), nsets, (u32 *)(A + o_cset));
        }
        fa.bm = (unsigned long long *)(A + o_bm);
        fa.owner[0] = (unsigned long long *)(A + o_ow0); fa.owner[1] = (unsigned long long *)(A + o_ow1);
        fa.tile_ptr = (const u32 *)(A + o_tptr);
        fa.tile_cnt[0] = (u32 *)(A + o_tc0); fa.tile_cnt[1] = (u32 *)(A + o_tc1);
        fa.xcd_tile = (const u32 *)(A + o_xt); fa.xcd_ntiles = (const u32 *)(A + o_xn);
        fa.set_ptr = (const u32 *)(A + o_sptr);
        fa.row_gs = (const u32 *)R->gs.p; fa.row_ge = (const u32 *)R->ge.p; fa.row_univ = (const i32 *)R->univ.p;
        fa.rows4 = (const uint4 *)R->rows4.p;
        if (direct) {
            // the buckets know where their sets' rows lie: nothing is searched in the rows
            fa.set_end = (const u32 *)(A + o_send);
            if (R->nb)
                hipLaunchKernelGGL(gr_set_range_kernel, dim3((unsigned)div_up((i64)R->nb, 256)), dim3(256), 0, s,
                                   (const u32 *)R->bstart.p, (const u32 *)R->mcnt.p, R->bucket_set, R->nb, nsets,
                                   (u32 *)(A + o_sptr), (u32 *)(A + o_send));
        } else {
            fa.set_end = fa.set_ptr + 1;
            hipLaunchKernelGGL(set_ptr_kernel, dim3((unsigned)div_up((i64)nsets + 1, 256)), dim3(256), 0, s, (const i32 *)R->set_id.p,
                               nrows, nsets, (u32 *)(A + o_sptr));
        }
        fa.rank = (const u32 *)(A + o_rank); fa.usize = (u32 *)(A + o_usize);
        fa.acc[0] = (u32 *)(A + o_acc0); fa.acc[1] = (u32 *)(A + o_acc1);
        fa.claimed = (u32 *)(A + o_claimed); fa.lost = (u32 *)(A + o_lost);
        fa.picked = (u32 *)(A + o_picked); fa.picks = (u32 *)(A + o_picks);
        fa.alive[0] = list_alive ? (u32 *)(A + o_al0) : nullptr; fa.alive[1] = list_alive ? (u32 *)(A + o_al1) : nullptr;
        fa.alive_cnt[0] = (u32 *)(A + o_alc0); fa.alive_cnt[1] = (u32 *)(A + o_alc1); fa.alive_seg = alive_seg;
        fa.pick_key = (unsigned long long *)(A + o_keys);
        fa.blkcnt = (unsigned long long *)(A + o_blk); fa.st = (GreedyState *)(A + o_st);
        fa.nsets = nsets; fa.nwords = (u32)nwords; fa.ntiles = nsub; fa.nuniv = nuniv;
        fa.nbands = nbands; fa.band_thr = (const u32 *)(A + o_thr); fa.band = nbands > 1 ? (const u8 *)(A + o_band) : nullptr;
        fa.set_thr = by_group ? (const u32 *)(A + o_sthr) : nullptr; fa.ngroups = ngroups;
        if (nbands > 1) {
            const u32 ng = std::min<u32>(R->gain0_n, nsets);
            const dim3 gmax_grid((unsigned)std::max<i64>(1, std::min<i64>(div_up((i64)ng, 1024), (i64)ctx->num_cus)));
            if (by_group)
                hipLaunchKernelGGL(gr_group_gain_max_kernel, gmax_grid, dim3(256), 0, s, (const u32 *)R->gain0.p, ng,
                                   (const u32 *)R->set_group.p, R->set_group_n, (u32 *)(A + o_gmax));
            else
                hipLaunchKernelGGL(gr_gain_max_kernel, gmax_grid, dim3(256), 0, s, (const u32 *)R->gain0.p, ng, (GreedyState *)(A + o_st));
            hipLaunchKernelGGL(gr_band_kernel, dim3((unsigned)div_up((i64)std::max(nsets, ngroups), 256)), dim3(256), 0, s,
                               (const u32 *)R->gain0.p, ng, nsets, (GreedyState *)(A + o_st), nbands, band_ratio, (u32 *)(A + o_thr),
                               (u8 *)(A + o_band), by_group ? (const u32 *)(A + o_gmax) : (const u32 *)(A + o_st + offsetof(GreedyState, gmax)),
                               ngroups, by_group ? (const u32 *)R->set_group.p : (const u32 *)nullptr, R->set_group_n,
                               by_group ? (u32 *)(A + o_sthr) : (u32 *)nullptr);
        } else hipLaunchKernelGGL(gr_fill_one_kernel, dim3(1), dim3(1), 0, s, (u32 *)(A + o_thr), 1u);
        fa.sharded = sharded ? 1u : 0u;
        fa.pretested = (sharded && partial) ? 1u : 0u;
        fa.changed[0] = stats_dirty ? (u32 *)(A + o_chg0) : nullptr; fa.changed[1] = stats_dirty ? (u32 *)(A + o_chg1) : nullptr;
        fa.nchg = (u32)nchg; fa.tile_shift = tile_shift;
        // rows into (tile, set, start) order: one stable partition by tile
        if (nrows) {
            const u32 nblk = (u32)div_up(src.n, GT_TILE);
            DevBuf<u32> hist, tmp;
            TRY(hist.alloc((size_t)nsub * nblk));
            hipLaunchKernelGGL(gr_tile_hist_kernel, dim3(nblk), dim3(GT_THREADS), 0, s, src, tile_shift, nsub, hist.p, nblk, fa.band, nbands);
            TRY(chip_exclusive_scan_u32(ctx, hist.p, hist.p, (i64)nsub * nblk, tmp));
            hipLaunchKernelGGL(gr_tile_scatter_kernel, dim3(nblk), dim3(GT_THREADS), 0, s, src, tile_shift, nsub,
                               (const u32 *)hist.p, nblk, (unsigned long long *)skey.p,
                               partial ? (const u32 *)(A + o_cflag) : (const u32 *)nullptr, partial ? suni.p : (u32 *)nullptr,
                               fa.band, nbands);
            hipLaunchKernelGGL(gr_tile_ptr_kernel, dim3(1), dim3(256), 0, s, (const u32 *)hist.p, nblk, nrows, nsub,
                               (u32 *)(A + o_tptr), fa.tile_cnt[0]);
            // (hist / tmp go back to the pool; their reuse is ordered by the stream)
        } else {
            hipLaunchKernelGGL(gr_tile_ptr_kernel, dim3(1), dim3(256), 0, s, (const u32 *)nullptr, 0u, 0u, nsub,
                               (u32 *)(A + o_tptr), fa.tile_cnt[0]);
        }
        hipLaunchKernelGGL(gr_tile_assign_kernel, dim3(1), dim3(256), 0, s, (const u32 *)fa.tile_cnt[0], ntiles, nbands,
                           (tile_shift >= 0 && !chip_test_env("CATCHHIP_FLAT_TILES_ROUND_ROBIN")) ? 1 : 0, (u32 *)(A + o_xt), (u32 *)(A + o_xn));
        // the sorted records are buffer 0, the sort's scratch is buffer 1
        fa.key[0] = (unsigned long long *)skey.p;
        fa.key[1] = (unsigned long long *)skey_alt.p;
        // Full coverage on one device needs no universe bitmap at all: every position of a row is in the universe
        // (the union of the rows), so a row's uncovered positions are those of its own that are not COVERED yet --
        // the bitmap holds the covered positions and starts empty (round 3: gr_bitmap was 5.9 ms per S4 step).
        // Partial coverage needs |U_u| per genome and a shard the all-reduced needs: those keep the union.
        fa.inv = (!partial && !sharded) ? ~0ull : 0ull;
        if (!fa.inv) hipLaunchKernelGGL(gr_bitmap_kernel, dim3(gblocks), dim3(GR_THREADS), 0, s, fa);
        // Round 0 of a full-coverage solve counts nothing that is not known: every row is uncovered, a set's gain is
        // the total length of its rows -- which the row build summed on the way (catchhip_rows::gain0).  Then the
        // first count launch (a pass over every record: 0.9 of the 21 ms of S4's largest solve) is left out.
        fa.count0_done = 0;
        if (!partial && !sharded && !stats_dirty && R->gain0_n && nrows && !chip_test_env("CATCHHIP_FLAT_COUNT_ROUND0")) {
            const u32 ng = std::min<u32>(R->gain0_n, nsets);
            HIP_TRY(hipMemcpyAsync(fa.acc[0], R->gain0.p, sizeof(u32) * (size_t)ng, hipMemcpyDeviceToDevice, s));
            hipLaunchKernelGGL(gr_fill_one_kernel, dim3(1), dim3(1), 0, s, fa.acc[0] + nsets, 1u);
            fa.count0_done = 1;
        }
        if (partial && nuniv) {
            // |U_u| -> what is left to cover of every universe; universes that need nothing drop out now
            hipLaunchKernelGGL(gf_universe_kernel, dim3(nuniv), dim3(256), 0, s, (const unsigned long long *)fa.bm,
                               (const u32 *)R->genome_off.p, fa.usize, fa.st, (const u32 *)nullptr);
            hipLaunchKernelGGL(gr_need_init_kernel, dim3((unsigned)div_up((i64)nuniv, 256)), dim3(256), 0, s,
                               (const u32 *)fa.usize, (const double *)d_p.p, nuniv, fa.need);
            launch_finish(0);
            if (tm) tm->launch(6);
        }
        if (tm) tm->launch(6);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // a round = count, claim, apply; under partial coverage: count, fixup (the complex sets' gains), claim,
    // usel (the universes' thresholds from this round's owner words), apply (with the universe test), finish
    void launch_count(u32 round) {
        if (round == 0 && fa.count0_done) return;      // (the gains of round 0 came with the rows)
        if (partial) {
            hipLaunchKernelGGL(gr_count_kernel<true>, dim3(gblocks), dim3(GR_THREADS), 0, ctx->stream, fa, round);
            hipLaunchKernelGGL(gr_fixup_kernel, dim3((unsigned)std::min<i64>(div_up((i64)nsets, 4), (i64)ctx->num_cus * 8)), dim3(256), 0,
                               ctx->stream, fa, round);
        } else if (round == 0 || fa.changed[0] || !fa.inv) {
            // round 0, the changed-word statistics, an uncovered bitmap (ranks): the instance that holds every path
            hipLaunchKernelGGL(gr_count_kernel<false>, dim3(gblocks), dim3(GR_THREADS), 0, ctx->stream, fa, round);
        } else {
            // the rounds of a full-coverage solve: the instance of its tile form, with or without gain bands
            const bool striped = fa.tile_shift < 0, banded = fa.nbands > 1;
            auto kern = striped ? (banded ? gr_count_kernel<false, true, GrForm<1, 1>> : gr_count_kernel<false, true, GrForm<1, 0>>)
                                : (banded ? gr_count_kernel<false, true, GrForm<0, 1>> : gr_count_kernel<false, true, GrForm<0, 0>>);
            hipLaunchKernelGGL(kern, dim3(gblocks), dim3(GR_THREADS), 0, ctx->stream, fa, round);
        }
    }
    void launch_claim(u32 round) {
        if (fa.set_thr) hipLaunchKernelGGL(gr_claim_kernel<true>, dim3(gblocks), dim3(GR_THREADS), 0, ctx->stream, fa, round);
        else hipLaunchKernelGGL(gr_claim_kernel<false>, dim3(gblocks), dim3(GR_THREADS), 0, ctx->stream, fa, round);
        if (partial && fa.nuniv) hipLaunchKernelGGL(gr_usel_kernel, dim3(fa.nuniv), dim3(256), 0, ctx->stream, fa, round);
    }
    void launch_verdict(u32 round) {
        hipLaunchKernelGGL(gr_verdict_kernel, dim3(gblocks), dim3(GA_THREADS), 0, ctx->stream, fa, round);
    }
    void launch_finish(u32 round) {
        hipLaunchKernelGGL(gr_finish_kernel, dim3((unsigned)div_up((i64)fa.nuniv, 4)), dim3(256), 0, ctx->stream, fa, round);
    }
    void launch_apply(u32 round) {
        if (partial) {
            hipLaunchKernelGGL(gr_apply_kernel<true>, dim3(gblocks), dim3(GA_THREADS), 0, ctx->stream, fa, round);
            if (fa.nuniv) launch_finish(round);
        } else {
            if (fa.set_thr) hipLaunchKernelGGL((gr_apply_kernel<false, true>), dim3(gblocks), dim3(GA_THREADS), 0, ctx->stream, fa, round);
            else hipLaunchKernelGGL(gr_apply_kernel<false>, dim3(gblocks), dim3(GA_THREADS), 0, ctx->stream, fa, round);
            hipLaunchKernelGGL(gr_cover_kernel, dim3(gblocks), dim3(GA_THREADS), 0, ctx->stream, fa, round);
        }
    }

    // picks in the sequential order (by rank, then by descending accept-time key)
    int picks(u32 np, const u32 *h_rank, i64 *out_ids) {
        hipStream_t s = ctx->stream;
        std::vector<u32> h_picks(np);
        std::vector<unsigned long long> h_keys(np);
        if (np) {
            HIP_TRY(hipMemcpyAsync(h_picks.data(), fa.picks, 4 * (size_t)np, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(h_keys.data(), fa.pick_key, 8 * (size_t)np, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        if (!h_rank) {
            // no ranks: the order is that of the keys alone, and a key names its set -- a byte-wise radix sort of
            // the keys (a comparison sort through an index array took milliseconds for the 100,000 picks of a
            // union instance)
            std::vector<unsigned long long> tmp(np);
            unsigned long long all_or = 0, all_and = ~0ull;
            for (u32 i = 0; i < np; ++i) { all_or |= h_keys[i]; all_and &= h_keys[i]; }
            for (int byte = 0; byte < 8; ++byte) {
                if ((((all_or ^ all_and) >> (8 * byte)) & 0xffull) == 0) continue;   // the same in every key
                size_t cnt[257] = {0};
                for (u32 i = 0; i < np; ++i) ++cnt[((h_keys[i] >> (8 * byte)) & 0xffull) + 1];
                for (int d = 0; d < 256; ++d) cnt[d + 1] += cnt[d];
                for (u32 i = 0; i < np; ++i) tmp[cnt[(h_keys[i] >> (8 * byte)) & 0xffull]++] = h_keys[i];
                h_keys.swap(tmp);
            }
            for (u32 i = 0; i < np; ++i) out_ids[i] = (i64)(ID_MASK - (u32)(h_keys[np - 1 - i] & ID_MASK));   // descending
            return 0;
        }
        std::vector<u32> ord(np);
        for (u32 i = 0; i < np; ++i) ord[i] = i;
        std::sort(ord.begin(), ord.end(), [&](u32 x, u32 y) {
            const u32 rx = h_rank ? h_rank[h_picks[x]] : 0u, ry = h_rank ? h_rank[h_picks[y]] : 0u;
            if (rx != ry) return rx < ry;
            return h_keys[x] > h_keys[y];
        });
        for (u32 i = 0; i < np; ++i) out_ids[i] = h_picks[ord[i]];
        return 0;
    }
};

static int greedy_flat(catchhip_ctx *ctx, const catchhip_rows *R, u32 nsets, const u32 *h_rank, u32 nrank,
                       i64 *out_ids, i64 *n_out, const double *h_p = nullptr) {
    hipStream_t s = ctx->stream;
    FlatSolve F;
    PhaseTimer tm(ctx, PHASE_GREEDY);
    TRY(F.setup(ctx, R, nsets, h_rank, nrank, false, &tm, h_p));
    const i64 max_rounds = (i64)nsets + nrank + 2 + F.fa.nbands;
    i64 rounds = 0;
    int per_sync = 16;   // most instances finish in 13-21 rounds: one or two synchronisations
    u8 *H = (u8 *)ctx->h_big;
    GreedyState *h_st = (GreedyState *)H;
    unsigned long long *h_blk = (unsigned long long *)(H + sizeof(GreedyState));
    PhaseTimer tr(ctx, PHASE_GREEDY_ROUNDS);
    // the claim launches alone (the largest kernel of a round): an event pair per launch, read at the
    // batch's synchronisation
    ctx->phase_ms[PHASE_CLAIM] = 0.0;
    ctx->phase_launches[PHASE_CLAIM] = 0;
    for (;;) {
        for (int r = 0; r < per_sync; ++r, ++rounds) {
            F.launch_count((u32)rounds);
            if (r < CHIP_EVX) (void)hipEventRecord(ctx->evx[2 * r], s);
            F.launch_claim((u32)rounds);
            if (r < CHIP_EVX) (void)hipEventRecord(ctx->evx[2 * r + 1], s);
            F.launch_apply((u32)rounds);
        }
        const int timed = std::min(per_sync, CHIP_EVX);
        tm.launch(3 * per_sync);
        tr.stop();
        tm.stop();
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_st, F.fa.st, sizeof(GreedyState), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h_blk, F.fa.blkcnt, 32 * (size_t)F.gblocks, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int r = 0; r < timed; ++r) {
            float ms = 0.f;
            // (timing is best effort: a pair that cannot be read adds nothing)
            if (hipEventElapsedTime(&ms, ctx->evx[2 * r], ctx->evx[2 * r + 1]) == hipSuccess) ctx->phase_ms[PHASE_CLAIM] += ms;
            ctx->phase_launches[PHASE_CLAIM]++;
        }
        if (h_st->done) break;
        if (rounds > max_rounds) { chip_set_error("setcover: round cap exceeded"); return CATCHHIP_EINVAL; }
        per_sync = F.partial ? 8 : 4;          // (partial coverage: ~100 rounds per large group, a host synchronisation each batch)
        tr.stopped = false;
        tm.stopped = false;
    }
    tr.launch(2 * rounds);   // reported in pairs, like the fused solver's rounds
    tr.finish();
    tm.finish();
    // row records streamed by the count launches / of those, rows whose words were read again / words read
    i64 n_vis = 0, n_rec = 0, n_wrd = 0, n_own = 0;
    for (unsigned b = 0; b < F.gblocks; ++b) {
        n_vis += (i64)h_blk[4 * b]; n_rec += (i64)h_blk[4 * b + 1]; n_wrd += (i64)h_blk[4 * b + 2]; n_own += (i64)h_blk[4 * b + 3];
    }
    ctx->solver_counters[0] = n_vis; ctx->solver_counters[1] = n_rec; ctx->solver_counters[2] = n_wrd; ctx->solver_counters[3] = n_own;
    const u32 np = h_st->npicks, iters = h_st->iters, done = h_st->done;
    ctx->phase_launches[PHASE_GREEDY] = iters;
    ctx->counters[2] = iters; ctx->counters[3] = np; ctx->counters[4] = n_vis;
    ctx->counters[5] = n_rec; ctx->counters[6] = n_wrd;
    ctx->solver_levels[0] = F.fa.nbands > 1 ? (i64)std::max(h_st->level[0], h_st->level[1]) + 1 : 1; ctx->solver_levels[1] = F.fa.nbands;
    ctx->solver_band_groups = F.fa.nbands > 1 ? (i64)std::max<u32>(h_st->band_groups, 1u) : 1;
    if (done == 2) {
        chip_set_error("setcover: ranks exhausted while coverage is still required");
        return CATCHHIP_ERANK;
    }
    TRY(F.picks(np, h_rank, out_ids));
    *n_out = np;
    return 0;
}
