// Frontier solver with the UNIVERSES sharded over ranks (included by setcover.hip).
//
// One set cover instance (one group) split over several GPUs: rank r holds a
// contiguous range of the group's genomes (= universes), has scanned ALL
// candidate probes against them and owns the cover rows that fall there; the
// set ids are the same on every rank.  Universes are disjoint, so
//   gain(s) = sum over ranks of the set's still-uncovered elements on that rank
// and the locally-maximal test of setcover_batched.inc ("s owns every bitmap
// word where it still has uncovered bits") is the AND over ranks of the same
// test on each rank's words.  A round therefore needs exactly two exchanges
// (BASELINE.json's "all-reduce of per-probe marginal coverage each greedy
// iteration" -- per ROUND of the frontier solver, not per pick):
//
//   count           local uncovered elements of every live set  -> acc[s]
//                   (+ acc[nsets] = local universes still in need)
//   all-reduce SUM  u32 gains                                   -> global gains
//   claim           key = (global gain, ~id); sets of the current rank raise
//                   owner[word] to their key on THEIR local words, the losers
//                   of a word are marked                         -> lost[s]
//   all-reduce MAX  u8 lost marks                               -> lost anywhere
//   apply           claimants that lost nowhere are accepted on every rank:
//                   clear the local bits, credit the local universes, record
//                   (set, key)
//
// The kernels are the row-parallel ones of setcover_flat.inc in their sharded
// mode (FlatArgs.sharded).  gain[], picked[], claimed[], the rank under
// consideration and the pick set are identical on all ranks after every round
// (they are functions of the all-reduced buffers only), so no further
// agreement is needed; the picks are put into the sequential order on the host
// by their keys, as in the unsharded solver.  Instances of at most 2^25 sets
// with rows of at most 257 bases; other groups are solved whole on one rank
// (catch_amd/parallel.py).  Partial coverage (p < 1): the universe test of a
// candidate runs on every rank over its own universes (gr_verdict_kernel) and
// failures travel as lost marks in a second exchange of that buffer before the
// apply launch (catchhip_shard_verdict).
//
// Packed exchange.  A set whose GLOBAL gain has reached zero never gains again,
// and only sets with a global gain can claim or lose: so the ranks exchange the
// gains and lost marks of the sets that were alive at the last read-back -- a
// list every rank derives from the same all-reduced gains, in set order (a set
// that has died since carries zeros).  On S4's largest group (3.96 M sets, 19
// rounds) that is ~4 x 16 MB of gains and ~4 x 4 MB of marks per solve instead
// of 19 x (16 + 16) MB.  Rounds are queued in batches (catchhip_shard_solve: as
// the unsharded solver queues them; the step API: batches of one round), the
// list is compacted once per batch from the all-reduced gains of its last round,
// and its new length comes back with the solver's state in the batch's one
// read-back.  The done flag stops the launches of rounds queued beyond the end;
// their collectives still run, on every rank alike (the batch length is the
// same everywhere).

// the most shards one process may exchange among themselves (their buffers travel as a kernel argument)
#define SHARD_LOCAL_MAX 64
struct ShardBufs { void *p[SHARD_LOCAL_MAX]; };

// n buffers of `count` elements on one device: every buffer <- reduction of all
template <typename T, bool IS_MAX>
__global__ void __launch_bounds__(256)
local_allreduce_kernel(ShardBufs bufs, int n, size_t count) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        T acc = ((const T *)bufs.p[0])[i];
        for (int b = 1; b < n; ++b) { const T v = ((const T *)bufs.p[b])[i]; acc = IS_MAX ? (v > acc ? v : acc) : (T)(acc + v); }
        for (int b = 0; b < n; ++b) ((T *)bufs.p[b])[i] = acc;
    }
}

// xg[i] = acc[list[i]] (list == null: i), xg[n], xg[n + 1] = the two extra slots
__global__ void __launch_bounds__(256)
sx_pack_gain_kernel(const u32 *__restrict__ acc, const u32 *__restrict__ list, u32 n, u32 nsets, u32 *__restrict__ xg) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) xg[i] = acc[list ? list[i] : i];
    else if (i < n + 2) xg[i] = acc[nsets + (i - n)];
}
// the all-reduced gains back into acc
__global__ void __launch_bounds__(256)
sx_unpack_gain_kernel(u32 *__restrict__ acc, const u32 *__restrict__ list, u32 n, u32 nsets, const u32 *__restrict__ xg) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) acc[list ? list[i] : i] = xg[i];
    else if (i < n + 2) acc[nsets + (i - n)] = xg[i];
}
// the lost marks of the listed sets, one byte each
__global__ void __launch_bounds__(256)
sxl_pack_lost_kernel(const u32 *__restrict__ lost, const u32 *__restrict__ list, u32 n, u32 tag, u8 *__restrict__ xl) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) xl[i] = lost[list ? list[i] : i] == tag ? 1 : 0;
}
__global__ void __launch_bounds__(256)
sxl_unpack_lost_kernel(u32 *__restrict__ lost, const u32 *__restrict__ list, u32 n, u32 tag, const u8 *__restrict__ xl) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && xl[i]) lost[list ? list[i] : i] = tag;
}
// flag[i] = set list[i] still has a global gain; flag[n] = 0 (its scanned slot receives the count)
__global__ void __launch_bounds__(256)
sx_flag_alive_kernel(const u32 *__restrict__ acc, const u32 *__restrict__ list, u32 n, u32 *__restrict__ flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = acc[list ? list[i] : i] ? 1u : 0u;
    else if (i == n) flag[n] = 0u;
}
// next list = the alive entries of this one, in order (pos = exclusive scan of flag)
__global__ void __launch_bounds__(256)
sx_compact_kernel(const u32 *__restrict__ list, u32 n, const u32 *__restrict__ flag, const u32 *__restrict__ pos,
                  u32 *__restrict__ next, u32 *__restrict__ n_next) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flag[i]) next[pos[i]] = list ? list[i] : i;
    if (i == 0) *n_next = pos[n];
}

struct catchhip_shard {
    catchhip_ctx *ctx = nullptr;
    FlatSolve F;                 // gains = acc[round & 1], lost marks = round tags, both u32
    std::vector<u32> h_rank;
    bool has_ranks = false;
    bool partial = false;        // some universe may stay partly uncovered: a third exchange per round (catchhip_shard_verdict)
    u32 nsets = 0;
    u32 round = 0;
    GreedyState h_st = {};       // as of the last read-back
    int done = 0;                // 1 finished, -1 rank list exhausted: the shard is spent
    // packed exchange: xg / xl are what the transports all-reduce
    DevBuf<u32> xg, xlist[2], xflag, xpos, xtmp;
    DevBuf<u8> xl;
    u32 cap = 0;                 // listed sets = the sets alive at the last read-back
    int lcur = -1;               // which of xlist holds the list (-1: every set, until the first read-back)

    const u32 *list() const { return lcur < 0 ? nullptr : xlist[lcur].p; }
    int lnext() const { return lcur < 0 ? 0 : lcur ^ 1; }
    // the exchange buffers as the transports see them; both sized by the list (gains: + 2 slots)
    void *xptr(i32 which) { return which == 0 ? (void *)xg.p : (void *)xl.p; }
    size_t xcount(i32 which) const { return which == 0 ? (size_t)cap + 2 : (size_t)cap; }
    size_t xelem(i32 which) const { return which == 0 ? 4 : 1; }
};

extern "C" int catchhip_shard_create_p(catchhip_ctx *ctx, const catchhip_rows *R, i64 num_sets, const i64 *ranks,
                                       const double *universe_p, catchhip_shard **out);
extern "C" int catchhip_shard_create_pi(catchhip_ctx *ctx, const catchhip_rows *R, i64 num_sets, const i64 *ranks,
                                        const double *universe_p, int instance_partial, catchhip_shard **out);
extern "C" int catchhip_shard_create(catchhip_ctx *ctx, const catchhip_rows *R, i64 num_sets, const i64 *ranks,
                                     catchhip_shard **out) {
    return catchhip_shard_create_p(ctx, R, num_sets, ranks, nullptr, out);
}

// universe_p: per LOCAL universe the fraction to cover (set_cover.py:362-373), or null = all of every universe
extern "C" int catchhip_shard_create_p(catchhip_ctx *ctx, const catchhip_rows *R, i64 num_sets, const i64 *ranks,
                                       const double *universe_p, catchhip_shard **out) {
    return catchhip_shard_create_pi(ctx, R, num_sets, ranks, universe_p, -1, out);
}

// instance_partial: whether ANY universe of the WHOLE instance (on any rank) is covered partially -- 1 / 0, the same
// on every rank, so that every rank takes the same shape of a round even when its own universes all have p == 1
// (coverage given in bases with genomes shorter than it: set_cover_filter.py:761-792); -1 = decide from this shard's
// universe_p alone (a single-shard caller).
extern "C" int catchhip_shard_create_pi(catchhip_ctx *ctx, const catchhip_rows *R, i64 num_sets, const i64 *ranks,
                                        const double *universe_p, int instance_partial, catchhip_shard **out) {
    ARG_CHECK(ctx && R && out && num_sets > 0 && R->ctx == ctx && !R->deferred);
    ARG_CHECK(instance_partial >= -1 && instance_partial <= 1);
    *out = nullptr;
    bool partial = false;
    if (universe_p)
        for (i64 u = 0; u < R->ngenomes; ++u) {
            ARG_CHECK(universe_p[u] >= 0.0 && universe_p[u] <= 1.0);
            partial = partial || universe_p[u] < 1.0;
        }
    if (instance_partial == 0 && partial) { chip_set_error("shard: a partial universe in an instance declared full"); return CATCHHIP_EINVAL; }
    std::vector<double> ones;
    if (instance_partial == 1) {
        partial = true;
        if (!universe_p) { ones.assign((size_t)std::max<i64>(R->ngenomes, 1), 1.0); universe_p = ones.data(); }
    }
    // (the caller -- every rank alike -- solves such a group whole)
    if (num_sets > (i64)GR_MAX_SETS || (R->n > 0 && R->lmax > 257)) {
        chip_set_error("shard: more than 2^%d sets or rows longer than 257 bases are solved unsharded", GR_SET_BITS);
        return CATCHHIP_EINVAL;
    }
    if (R->n >= ((i64)1 << 31)) { chip_set_error("shard: too many rows"); return CATCHHIP_EINVAL; }
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope pool_scope(ctx);
    std::unique_ptr<catchhip_shard> S(new catchhip_shard());
    S->ctx = ctx;
    const u32 nsets = (u32)num_sets;
    const u32 nrank = dense_ranks(ranks, nsets, S->h_rank);
    S->has_ranks = ranks != nullptr;
    S->partial = partial;
    S->nsets = S->cap = nsets;
    // everything a round or a batch needs is allocated here: nothing can fail to allocate between two collectives
    TRY(S->F.setup(ctx, R, nsets, S->has_ranks ? S->h_rank.data() : nullptr, nrank, true, nullptr,
                   partial ? universe_p : nullptr));
    TRY(S->xg.alloc((size_t)nsets + 2));
    TRY(S->xl.alloc((size_t)nsets + 16));
    TRY(S->xlist[0].alloc(nsets));
    TRY(S->xlist[1].alloc(nsets));
    TRY(S->xflag.alloc((size_t)nsets + 1));
    TRY(S->xpos.alloc((size_t)nsets + 1));
    TRY(chip_exclusive_scan_reserve(S->xtmp, (i64)nsets + 1));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *out = S.release();
    return 0;
}

extern "C" int catchhip_shard_destroy(catchhip_shard *S) {
    if (S) {
        (void)hipSetDevice(S->ctx->device);
        PoolScope pool_scope(S->ctx);
        delete S;
    }
    return 0;
}

// ---- the phases of a round and the end of a batch: the step API and catchhip_shard_solve run the same ones --------
#define SX_GRID(n) dim3((unsigned)div_up((i64)(n), 256)), dim3(256), 0, S->ctx->stream

// count + pack the gains
static void shard_count(catchhip_shard *S) {
    S->F.launch_count(S->round);
    hipLaunchKernelGGL(sx_pack_gain_kernel, SX_GRID((i64)S->cap + 2), (const u32 *)S->F.fa.acc[S->round & 1], S->list(),
                       S->cap, S->nsets, S->xg.p);
}

// the all-reduced gains back into place + claim + pack the lost marks
static void shard_claim(catchhip_shard *S) {
    hipLaunchKernelGGL(sx_unpack_gain_kernel, SX_GRID((i64)S->cap + 2), S->F.fa.acc[S->round & 1], S->list(), S->cap,
                       S->nsets, (const u32 *)S->xg.p);
    S->F.launch_claim(S->round);
    if (S->cap)
        hipLaunchKernelGGL(sxl_pack_lost_kernel, SX_GRID(S->cap), (const u32 *)S->F.fa.lost, S->list(), S->cap,
                           S->round + 1, S->xl.p);
}

// partial coverage: the all-reduced marks back into place + the universe test of every candidate left on this
// rank's universes (a failure is one more lost mark) + pack the marks again
static void shard_verdict(catchhip_shard *S) {
    if (S->cap)
        hipLaunchKernelGGL(sxl_unpack_lost_kernel, SX_GRID(S->cap), S->F.fa.lost, S->list(), S->cap, S->round + 1,
                           (const u8 *)S->xl.p);
    S->F.launch_verdict(S->round);
    if (S->cap)
        hipLaunchKernelGGL(sxl_pack_lost_kernel, SX_GRID(S->cap), (const u32 *)S->F.fa.lost, S->list(), S->cap,
                           S->round + 1, S->xl.p);
}

// the all-reduced marks back into place + apply; the round is over
static void shard_apply(catchhip_shard *S) {
    if (S->cap)
        hipLaunchKernelGGL(sxl_unpack_lost_kernel, SX_GRID(S->cap), S->F.fa.lost, S->list(), S->cap, S->round + 1,
                           (const u8 *)S->xl.p);
    S->F.launch_apply(S->round);
    S->round++;
}

// The end of a batch, enqueued: the list compacted to the sets that still have a global gain (the all-reduced gains
// of the batch's last round: the same on every rank); its length lands in the scanned flag slot.
static int shard_compact(catchhip_shard *S) {
    const u32 *lp = S->list();
    hipLaunchKernelGGL(sx_flag_alive_kernel, SX_GRID((i64)S->cap + 1), (const u32 *)S->F.fa.acc[(S->round - 1) & 1], lp,
                       S->cap, S->xflag.p);
    TRY(chip_exclusive_scan_u32(S->ctx, S->xflag.p, S->xpos.p, (i64)S->cap + 1, S->xtmp));   // (scratch reserved at creation)
    hipLaunchKernelGGL(sx_compact_kernel, SX_GRID(std::max<u32>(S->cap, 1)), lp, S->cap, (const u32 *)S->xflag.p,
                       (const u32 *)S->xpos.p, S->xlist[S->lnext()].p, S->xflag.p + S->cap);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ... and its one read-back: the solver's state and the list's new length, published unless the solve has ended
// (the rounds queued past the end did nothing: their list is not one to continue from)
static int shard_read_back(catchhip_shard *S) {
    catchhip_ctx *c = S->ctx;
    static_assert(sizeof(GreedyState) + sizeof(u32) <= 64 * sizeof(u64), "ctx->h_pin holds the state and one more word");
    u32 *h_n = (u32 *)((u8 *)c->h_pin + sizeof(GreedyState));
    HIP_TRY(hipMemcpyAsync(c->h_pin, S->F.fa.st, sizeof(GreedyState), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h_n, S->xflag.p + S->cap, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(&S->h_st, c->h_pin, sizeof(GreedyState));
    S->done = S->h_st.done == 2 ? -1 : (S->h_st.done ? 1 : 0);
    if (S->done) return 0;
    S->cap = *(volatile u32 *)h_n;
    S->lcur = S->lnext();
    if ((i64)S->round > 2 * (i64)S->nsets + 4) {      // (a round accepts a set or moves on to the next rank)
        chip_set_error("shard: round cap exceeded");
        return CATCHHIP_EINVAL;
    }
    return 0;
}

// One all-reduce of every shard's buffer `which` (0: gains, SUM; 1: lost marks, MAX) at its current size: over the
// context's communicator (transport 0: one shard per process) or among the n shards of this process (transport 1:
// one device, on shards[0]'s stream).  Allocates nothing.
static int shard_exchange(i32 n, catchhip_shard *const *sh, i32 which, i32 transport) {
    const size_t count = sh[0]->xcount(which);
    if (count == 0) return 0;      // (the same on every rank: the lists derive from the all-reduced gains)
    catchhip_ctx *c = sh[0]->ctx;
    if (transport == 0) {
        void *buf = sh[0]->xptr(which);
        const ncclResult_t r = which == 0 ? rccl().AllReduce(buf, buf, count, ncclUint32, ncclSum, (ncclComm_t)c->comm, c->stream)
                                          : rccl().AllReduce(buf, buf, count, ncclUint8, ncclMax, (ncclComm_t)c->comm, c->stream);
        if (r != ncclSuccess) { chip_set_error("ncclAllReduce: %s", rccl().GetErrorString(r)); return CATCHHIP_ECOMM; }
        return 0;
    }
    if (n == 1) return 0;
    ShardBufs b;
    for (i32 i = 0; i < n; ++i) b.p[i] = sh[i]->xptr(which);
    const unsigned blocks = (unsigned)std::min<size_t>(div_up((i64)count, 256), 4096);
    if (which == 0) hipLaunchKernelGGL((local_allreduce_kernel<u32, false>), dim3(blocks), dim3(256), 0, c->stream, b, n, count);
    else hipLaunchKernelGGL((local_allreduce_kernel<u8, true>), dim3(blocks), dim3(256), 0, c->stream, b, n, count);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the step API: a batch of one round --------------------------------------------------------------------------
static int shard_step_check(catchhip_shard *S) {
    ARG_CHECK(S != nullptr);
    if (S->done) { chip_set_error("shard: the solve has ended (a shard is single-use)"); return CATCHHIP_EINVAL; }
    HIP_TRY(hipSetDevice(S->ctx->device));
    return 0;
}

extern "C" int catchhip_shard_count(catchhip_shard *S) {
    TRY(shard_step_check(S));
    shard_count(S);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int catchhip_shard_buffers(catchhip_shard *S, void **gain, i64 *gain_count, void **lost, i64 *lost_count) {
    ARG_CHECK(S && gain && gain_count && lost && lost_count);
    *gain_count = (i64)S->xcount(0);
    *lost_count = (i64)S->xcount(1);
    *gain = S->xptr(0);
    *lost = S->xptr(1);
    return 0;
}

extern "C" int catchhip_shard_claim_check(catchhip_shard *S) {
    TRY(shard_step_check(S));
    shard_claim(S);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Partial coverage only, between the lost exchange and catchhip_shard_apply; the caller exchanges the marks once
// more (which = 1), then applies.
extern "C" int catchhip_shard_verdict(catchhip_shard *S) {
    TRY(shard_step_check(S));
    if (!S->partial) return 0;
    shard_verdict(S);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the end of the round and of its batch: the one host synchronisation of a round
extern "C" int catchhip_shard_apply(catchhip_shard *S, i32 *done) {
    ARG_CHECK(done != nullptr);
    TRY(shard_step_check(S));
    PoolScope pool_scope(S->ctx);
    shard_apply(S);
    TRY(shard_compact(S));
    TRY(shard_read_back(S));
    *done = S->done;
    return 0;
}

extern "C" int catchhip_shard_picks(catchhip_shard *S, i64 *out_ids, i64 *n_out) {
    ARG_CHECK(S && n_out);
    HIP_TRY(hipSetDevice(S->ctx->device));
    if (S->done == -1) { chip_set_error("setcover: ranks exhausted while coverage is still required"); return CATCHHIP_ERANK; }
    const u32 np = S->h_st.npicks;     // (the state of the last read-back: every apply is followed by one)
    *n_out = np;
    if (!np) return 0;
    ARG_CHECK(out_ids != nullptr);
    TRY(S->F.picks(np, S->has_ranks ? S->h_rank.data() : nullptr, out_ids));
    S->ctx->counters[2] = S->h_st.iters; S->ctx->counters[3] = np;
    return 0;
}

// out4 = {gain elements (uint32) and lost elements (uint8) of the NEXT exchange -- the buffers are packed, so the
// counts change from batch to batch --, bytes per lost element, 1 | 2 if partial}
extern "C" int catchhip_shard_info(catchhip_shard *S, i64 *out4) {
    ARG_CHECK(S && out4);
    out4[0] = (i64)S->xcount(0); out4[1] = (i64)S->xcount(1); out4[2] = 1; out4[3] = 1 | (S->partial ? 2 : 0);
    return 0;
}

// copy an exchange buffer to / from the host (transport of the caller's own,
// e.g. the gloo fallback of catch_amd/parallel.py when RCCL is not usable)
extern "C" int catchhip_shard_buffer_copy(catchhip_shard *S, i32 which, void *host, i32 to_host) {
    ARG_CHECK(S && host && (which == 0 || which == 1));
    HIP_TRY(hipSetDevice(S->ctx->device));
    void *dev = S->xptr(which);
    const size_t bytes = S->xelem(which) * S->xcount(which);
    if (bytes == 0) return 0;
    HIP_TRY(hipMemcpyAsync(to_host ? host : dev, to_host ? dev : host, bytes,
                           to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, S->ctx->stream));
    HIP_TRY(hipStreamSynchronize(S->ctx->stream));
    return 0;
}

// exchange between shards that live in one process on one device
extern "C" int catchhip_shard_allreduce_local(i32 n, catchhip_shard *const *shards, i32 which) {
    ARG_CHECK(n >= 1 && n <= SHARD_LOCAL_MAX && shards && (which == 0 || which == 1));
    for (i32 i = 0; i < n; ++i) {
        ARG_CHECK(shards[i] != nullptr && shards[i]->nsets == shards[0]->nsets);
        if (shards[i]->ctx->device != shards[0]->ctx->device) {
            chip_set_error("shard_allreduce_local: shards must be on one device (use RCCL across devices)");
            return CATCHHIP_EINVAL;
        }
        if (shards[i]->round != shards[0]->round || shards[i]->xcount(which) != shards[0]->xcount(which)) {
            chip_set_error("shard_allreduce_local: the shards disagree on the round or the size of the exchange");
            return CATCHHIP_EINVAL;
        }
    }
    catchhip_ctx *c0 = shards[0]->ctx;
    HIP_TRY(hipSetDevice(c0->device));
    for (i32 i = 0; i < n; ++i) HIP_TRY(hipStreamSynchronize(shards[i]->ctx->stream));
    TRY(shard_exchange(n, shards, which, 1));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    return 0;
}

// exchange over the context's RCCL communicator (one process per GPU)
extern "C" int catchhip_shard_allreduce(catchhip_shard *S, i32 which) {
    ARG_CHECK(S && (which == 0 || which == 1));
    if (!S->ctx->comm) { chip_set_error("shard_allreduce: no communicator (catchhip_comm_init)"); return CATCHHIP_ECOMM; }
    HIP_TRY(hipSetDevice(S->ctx->device));
    return shard_exchange(1, &S, which, 0);
}

// ---- the round loop under the C ABI (round 6) -------------------------------------------------------------------------
// Runs the instance to its end, rounds_per_sync >= 1 rounds per read-back.  shards: the n shards THIS process holds
// (transport 0 = RCCL over the context's communicator: n == 1; transport 1 = the shards exchange among themselves: one
// context).  *done: 1 finished, -1 the rank list ran out (catchhip_shard_picks then reports it).
extern "C" int catchhip_shard_solve(i32 n, catchhip_shard *const *shards, i32 transport, i32 rounds_per_sync, i32 *done) {
    ARG_CHECK(n >= 1 && n <= SHARD_LOCAL_MAX && shards && done && (transport == 0 || transport == 1) && rounds_per_sync >= 1);
    catchhip_shard *S0 = shards[0];
    ARG_CHECK(S0 != nullptr);
    catchhip_ctx *c = S0->ctx;
    for (i32 i = 0; i < n; ++i) {
        ARG_CHECK(shards[i] != nullptr && shards[i]->nsets == S0->nsets);
        if (shards[i]->ctx != c || shards[i]->partial != S0->partial || shards[i]->round != 0) {
            chip_set_error("shard_solve: the shards of one process share a context, the coverage and start at round 0");
            return CATCHHIP_EINVAL;
        }
    }
    if (transport == 0 && (n != 1 || !c->comm)) { chip_set_error("shard_solve: RCCL needs one shard per process and a communicator"); return CATCHHIP_ECOMM; }
    HIP_TRY(hipSetDevice(c->device));
    PoolScope pool_scope(c);
    for (;;) {
        for (i32 r = 0; r < rounds_per_sync; ++r) {
            for (i32 i = 0; i < n; ++i) shard_count(shards[i]);
            TRY(shard_exchange(n, shards, 0, transport));
            for (i32 i = 0; i < n; ++i) shard_claim(shards[i]);
            TRY(shard_exchange(n, shards, 1, transport));
            if (S0->partial) {
                for (i32 i = 0; i < n; ++i) shard_verdict(shards[i]);
                TRY(shard_exchange(n, shards, 1, transport));
            }
            for (i32 i = 0; i < n; ++i) shard_apply(shards[i]);
        }
        for (i32 i = 0; i < n; ++i) TRY(shard_compact(shards[i]));
        for (i32 i = 0; i < n; ++i) {
            TRY(shard_read_back(shards[i]));
            if (shards[i]->done != S0->done || shards[i]->cap != S0->cap) {
                chip_set_error("shard_solve: shards disagree (alive sets or termination)");
                return CATCHHIP_EINVAL;
            }
        }
        if (S0->done) { *done = S0->done; return 0; }
    }
}
