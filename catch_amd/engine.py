"""Thin Python objects over the C-ABI handles of libcatchhip.so.

Only marshals NumPy host buffers in and out (stdlib + NumPy, no torch); all
compute happens in the HIP kernels behind include/catchhip.h.
"""
import ctypes

import numpy as np

from catch_amd import _lib
from catch_amd._lib import (c_f32p, c_f64p, c_i32p, c_i64p, c_u16p, c_u32p,
                            c_u64p, c_u8p, check)

SCAN_AUTO, SCAN_GENERAL, SCAN_FAST, SCAN_SEED = 0, 1, 2, 3
PHASE_SCAN, PHASE_ROWS, PHASE_GREEDY, PHASE_NDF, PHASE_GREEDY_ROUNDS = 0, 1, 2, 3, 4
PHASE_VERIFY = 5
PHASE_CLAIM = 6
PHASE_VCOUNT = 7      # key-grouped join: the counting pass (PHASE_VERIFY: the writing pass)
PHASE_POOL = 8        # catchhip_pool_solve: one launch per dataset + the walk back


def _ptr(a, t):
    return a.ctypes.data_as(t)


def _concat(strs):
    off = np.zeros(len(strs) + 1, dtype=np.int64)
    if strs:
        np.cumsum([len(s) for s in strs], out=off[1:])
    buf = np.frombuffer("".join(strs).encode("latin-1"), dtype=np.uint8)
    if buf.size == 0:
        buf = np.zeros(1, dtype=np.uint8)
    return np.ascontiguousarray(buf), off


_as_utf8 = None


def _str_pointers(strs):
    """(void*[n], int64 lengths) of the strings' own byte storage, or None when
    some string is not plain ASCII (then the caller concatenates instead).
    CPython keeps an ASCII str as one byte per character and
    PyUnicode_AsUTF8AndSize hands out that buffer without a copy; it stays valid
    while the str is alive, i.e. for the duration of the call it is passed to."""
    global _as_utf8
    if isinstance(strs, FragmentTable):
        return strs.pointers()
    if _as_utf8 is None:
        _as_utf8 = ctypes.pythonapi.PyUnicode_AsUTF8AndSize
        _as_utf8.restype = ctypes.c_void_p
        _as_utf8.argtypes = [ctypes.py_object, ctypes.POINTER(ctypes.c_ssize_t)]
    n = len(strs)
    arr = (ctypes.c_void_p * n)()
    lens = np.zeros(n, dtype=np.int64)
    size = ctypes.c_ssize_t(0)
    ref = ctypes.byref(size)
    for i, s in enumerate(strs):
        if not isinstance(s, str) or not s.isascii():
            return None
        arr[i] = _as_utf8(s, ref)
        lens[i] = size.value
    return arr, lens


class FragmentTable:
    """Sequences as VIEWS of their parents' own byte storage: (address, length) per fragment, the parents kept alive
    beside them.  A clustered design cuts 3.5 Gbases of genomes into 224 k fragments (catch/filter/probe_designer.py:
    78-184 via Genome.break_into_fragments); slicing them out as str objects and wrapping each in a Genome cost 0.6 s of
    a 4.3-s step before a single base was looked at, although everything downstream -- the signatures, the targets of
    the clusters -- only ever hands (pointer, length) pairs to the library.  `parents`: plain-ASCII str objects
    (others: build() returns None and the caller slices as before); fragment i = parents[parent[i]][start[i] :
    start[i] + length[i]]."""

    def __init__(self, parents, parent, start, length, addr):
        self.parents, self.parent, self.start, self.length, self.addr = parents, parent, start, length, addr

    @staticmethod
    def build(parents, parent, start, length):
        global _as_utf8
        if _as_utf8 is None:
            _as_utf8 = ctypes.pythonapi.PyUnicode_AsUTF8AndSize
            _as_utf8.restype = ctypes.c_void_p
            _as_utf8.argtypes = [ctypes.py_object, ctypes.POINTER(ctypes.c_ssize_t)]
        n = len(parents)
        if n and (set(map(type, parents)) != {str} or not all(map(str.isascii, parents))):
            return None
        base = np.zeros(max(n, 1), dtype=np.uint64)
        size = ctypes.c_ssize_t(0)
        ref = ctypes.byref(size)
        # A plain-ASCII str keeps its characters right behind its header (CPython's "compact ASCII" layout), so the
        # address is id(s) + the header's size -- one vectorised add instead of 198 k calls through ctypes (0.2 s of a
        # 4.3-s step).  The header size is MEASURED on this interpreter, and the first and last parents are checked
        # against PyUnicode_AsUTF8AndSize; any surprise falls back to the call per string.
        fast = False
        if n:
            probe_s = "ACGT" * 3
            hdr = _as_utf8(probe_s, ref) - id(probe_s)
            if 0 < hdr <= 128:
                base[:n] = np.fromiter(map(id, parents), dtype=np.uint64, count=n) + np.uint64(hdr)
                fast = all(int(base[i]) == _as_utf8(parents[i], ref) for i in {0, n // 2, n - 1})
        if not fast:
            for i, s in enumerate(parents):
                base[i] = _as_utf8(s, ref)
        parent = np.ascontiguousarray(parent, dtype=np.int64)
        start = np.ascontiguousarray(start, dtype=np.int64)
        length = np.ascontiguousarray(length, dtype=np.int64)
        return FragmentTable(parents, parent, start, length, base[parent] + start.astype(np.uint64))

    def __len__(self):
        return int(self.length.size)

    def take(self, idx):
        """The fragments idx (an index array), in that order."""
        idx = np.asarray(idx, dtype=np.int64)
        return FragmentTable(self.parents, self.parent[idx], self.start[idx], self.length[idx], self.addr[idx])

    def string(self, i, lo=0, hi=None):
        """Fragment i (or its characters [lo, hi)) as a str."""
        a = int(self.start[i])
        b = a + int(self.length[i])
        return self.parents[int(self.parent[i])][a + lo:b if hi is None else a + hi]

    def pointers(self):
        """(void*[n], int64 lengths) as _str_pointers gives them."""
        arr = (ctypes.c_void_p * max(len(self), 1)).from_buffer_copy(
            np.ascontiguousarray(self.addr if len(self) else np.zeros(1, dtype=np.uint64)).tobytes())
        return arr, np.ascontiguousarray(self.length)


def pyset_order(hashes):
    """catchhip_pyset_order: indices in the order a CPython set iterates keys
    with these hashes after they were added in index order."""
    h = np.ascontiguousarray(hashes, dtype=np.int64)
    out = np.zeros(max(h.size, 1), dtype=np.int64)
    check(_lib.lib().catchhip_pyset_order(_ptr(h, c_i64p), int(h.size), _ptr(out, c_i64p)))
    return out[:h.size]


def pyset_order_strs(strs):
    """catchhip_pyset_order_strs: the order `list(set)` would give the distinct
    ASCII strings after they were added one by one (hash(str) of CPython <=
    3.10 under PYTHONHASHSEED=0)."""
    n = len(strs)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    buf, off = _concat(strs)
    out = np.zeros(n, dtype=np.int64)
    check(_lib.lib().catchhip_pyset_order_strs(_ptr(buf, c_u8p), _ptr(off, c_i64p), n, _ptr(out, c_i64p)))
    return out


def device_count():
    n = ctypes.c_int(0)
    rc = _lib.lib().catchhip_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def pool_trim():
    """catchhip_pool_trim: idle cached device blocks go back to the driver."""
    check(_lib.lib().catchhip_pool_trim())


def pool_stats():
    """catchhip_pool_stats -> dict (device-memory cache of the library)."""
    out = np.zeros(4, dtype=np.int64)
    check(_lib.lib().catchhip_pool_stats(_ptr(out, c_i64p)))
    return dict(zip(("hipmalloc_calls", "bytes_held", "bytes_cached_free",
                     "oom_retries"), (int(x) for x in out)))


class Context:
    """One HIP device + stream (catchhip_ctx)."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        self._L = _lib.lib()
        check(self._L.catchhip_ctx_create(int(device), ctypes.byref(self._h)))
        self.device = int(device)

    def close(self):
        """Destroys the context.  An object made on it that is still open is not destroyed afterwards (its device
        memory stays allocated): the garbage collector may finalize a context before such objects when they are
        part of one cycle (e.g. the frame of a failed test), and their destroy calls would read the freed context."""
        if self._h:
            self._L.catchhip_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self._L.catchhip_ctx_sync(self._h))

    def kernel_ms(self, phase):
        ms = ctypes.c_double(0.0)
        n = ctypes.c_int64(0)
        check(self._L.catchhip_ctx_last_kernel_ms(self._h, phase,
                                                  ctypes.byref(ms),
                                                  ctypes.byref(n)))
        return ms.value, n.value

    def counters(self):
        """catchhip_ctx_last_counters -> dict of work counters."""
        out = np.zeros(8, dtype=np.int64)
        check(self._L.catchhip_ctx_last_counters(self._h, _ptr(out, c_i64p)))
        names = ["raw_hits", "seed_hits", "greedy_iters", "picks",
                 "winner_rows", "rows_recounted", "bitmap_words_read", "_"]
        d = dict(zip(names, (int(x) for x in out)))
        dropped = np.zeros(1, dtype=np.int64)
        check(self._L.catchhip_ctx_last_seeds_dropped(self._h, _ptr(dropped, c_i64p)))
        d["seeds_dropped"] = int(dropped[0])   # of seed_hits: left without a seed by the look-up's filter
        check(self._L.catchhip_ctx_last_rows_direct(self._h, _ptr(dropped, c_i64p)))
        d["rows_direct"] = int(dropped[0])     # 1: the last setcover_filter solved from the bucketed records
        jc = np.zeros(4, dtype=np.int64)
        check(self._L.catchhip_ctx_last_join_counters(self._h, _ptr(jc, c_i64p)))
        d.update(zip(("join_hit_positions", "join_pairs", "join_lane_slots", "join_cut_tasks"), (int(x) for x in jc)))
        sc = np.zeros(4, dtype=np.int64)
        check(self._L.catchhip_ctx_last_solver_counters(self._h, _ptr(sc, c_i64p)))
        d.update(zip(("flat_rows_streamed", "flat_rows_recounted", "flat_bitmap_words",
                      "flat_owner_words"), (int(x) for x in sc)))
        lv = np.zeros(2, dtype=np.int64)
        check(self._L.catchhip_ctx_last_solver_levels(self._h, _ptr(lv, c_i64p)))
        d["flat_levels"], d["flat_bands"] = int(lv[0]), int(lv[1])   # gain bands of the last row-parallel solve
        check(self._L.catchhip_ctx_last_solver_band_groups(self._h, _ptr(lv, c_i64p)))
        d["flat_band_groups"] = int(lv[0])   # groups with band boundaries of their own (1: one row of boundaries)
        return d

    CAPACITY_EVENTS = ("seed_list_rerun", "general_seed_rerun", "byte_join_rerun", "fast_hit_rerun",
                       "cut_list_fallback", "giant_task_fallback", "ndf_edge_rerun", "_")

    def capacity_events(self):
        """catchhip_ctx_last_capacity_events -> dict: how often the last scan or near-duplicate filter on this
        context found a device buffer too small and ran again at the exact size (or took the slower path)."""
        out = np.zeros(8, dtype=np.int64)
        check(self._L.catchhip_ctx_last_capacity_events(self._h, _ptr(out, c_i64p)))
        return dict(zip(self.CAPACITY_EVENTS, (int(x) for x in out)))

    def grid_counters(self):
        """catchhip_ctx_last_grid_counters of the last setcover_grid call."""
        out = np.zeros(4, dtype=np.int64)
        check(self._L.catchhip_ctx_last_grid_counters(self._h, _ptr(out, c_i64p)))
        return dict(zip(("scans", "derived", "solves", "rows0"), (int(x) for x in out)))

    def pyset_order(self, hashes):
        """catchhip_pyset_order_device: engine.pyset_order computed on the device."""
        h = np.ascontiguousarray(hashes, dtype=np.int64)
        out = np.zeros(max(h.size, 1), dtype=np.int64)
        check(self._L.catchhip_pyset_order_device(self._h, _ptr(h, c_i64p), int(h.size), _ptr(out, c_i64p)))
        return out[:h.size]

    def ndf_counters(self):
        """catchhip_ctx_last_ndf_counters -> dict (last Hamming filter)."""
        out = np.zeros(4, dtype=np.int64)
        check(self._L.catchhip_ctx_last_ndf_counters(self._h, _ptr(out, c_i64p)))
        return dict(zip(("probes", "tables", "pairs_compared", "edges"),
                        (int(x) for x in out)))

    # -- RCCL -----------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = np.zeros(128, dtype=np.uint8)
        check(_lib.lib().catchhip_comm_unique_id(_ptr(buf, c_u8p)))
        return buf.tobytes()

    @staticmethod
    def comm_info():
        """catchhip_comm_info: the RCCL copy (version, file) communicators use."""
        buf = ctypes.create_string_buffer(1024)
        check(_lib.lib().catchhip_comm_info(buf, 1024))
        return buf.value.decode("utf-8", "replace")

    def comm_init(self, unique_id, nranks, rank):
        import os
        import sys
        buf = np.frombuffer(unique_id, dtype=np.uint8).copy()
        # RCCL prints a version banner on stdout at first use; keep stdout
        # clean for callers that emit machine-readable output
        sys.stdout.flush()
        saved = os.dup(1)
        try:
            os.dup2(2, 1)
            rc = self._L.catchhip_comm_init(self._h, _ptr(buf, c_u8p), nranks,
                                            rank)
            ctypes.CDLL(None).fflush(None)   # the banner sits in C stdio's buffer
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        check(rc)

    def comm_destroy(self):
        check(self._L.catchhip_comm_destroy(self._h))

    def comm_selftest(self, nelem=1 << 20):
        """catchhip_comm_selftest: a checked SUM all-reduce on this context's communicator (collective)."""
        check(self._L.catchhip_comm_selftest(self._h, int(nelem)))

    # -- test entry points of the device-wide primitives (tests/test_primitives.py) ---
    def selftest_scan_u32(self, values, in_place=False):
        """catchhip_selftest_scan_u32: the device's exclusive prefix sum (mod 2^32) of uint32 values."""
        x = np.ascontiguousarray(values, dtype=np.uint32)
        out = np.zeros(max(x.size, 1), dtype=np.uint32)
        check(self._L.catchhip_selftest_scan_u32(self._h, _ptr(x, c_u32p), int(x.size), int(bool(in_place)),
                                                 _ptr(out, c_u32p)))
        return out[:x.size]

    def selftest_sort_pairs(self, keys, vals, key_bits, first_bit=0, nseg=0):
        """catchhip_selftest_sort_pairs: (keys, vals) as the device's radix sort leaves them.  nseg = 0: one sort
        of all pairs; nseg >= 1: keys / vals are nseg segments of equal length, each sorted on its own."""
        k = np.array(keys, dtype=np.uint64, order="C").reshape(-1)
        v = np.array(vals, dtype=np.uint32, order="C").reshape(-1)
        if k.size != v.size or (nseg > 0 and k.size % nseg):
            raise ValueError("selftest_sort_pairs: keys and vals must be nseg segments of one length")
        n = k.size // nseg if nseg > 0 else k.size
        check(self._L.catchhip_selftest_sort_pairs(self._h, _ptr(k, c_u64p), _ptr(v, c_u32p), int(n), int(nseg),
                                                   int(key_bits), int(first_bit)))
        return k, v

    WAVE_RESULTS_32 = ("wave_sum", "wave_max", "wave_sum_all", "wave_max_all", "wave_incl_scan", "wave_excl_scan",
                       "wave_excl_scan_total", "wave_incl_scan_dpp", "quad_sum", "row8_sum")
    WAVE_RESULTS_64 = ("wave_max_u64", "wave_incl_scan_u64")

    def selftest_wave(self, values):
        """catchhip_selftest_wave: what every helper of csrc/wave.h returned to every thread, by name; one uint32
        value per thread, a multiple of 256 of them."""
        x = np.ascontiguousarray(values, dtype=np.uint32)
        o32 = np.zeros((len(self.WAVE_RESULTS_32), x.size), dtype=np.uint32)
        o64 = np.zeros((len(self.WAVE_RESULTS_64), x.size), dtype=np.uint64)
        check(self._L.catchhip_selftest_wave(self._h, _ptr(x, c_u32p), int(x.size), _ptr(o32, c_u32p),
                                             _ptr(o64, c_u64p)))
        out = dict(zip(self.WAVE_RESULTS_32, o32))
        out.update(zip(self.WAVE_RESULTS_64, o64))
        return out

    def selftest_find_segment(self, off, x):
        """catchhip_selftest_find_segment: the device's find_segment(off, len(off) - 1, x[j]) for every j."""
        off = np.ascontiguousarray(off, dtype=np.uint32)
        x = np.ascontiguousarray(x, dtype=np.uint32)
        out = np.zeros(max(x.size, 1), dtype=np.uint32)
        check(self._L.catchhip_selftest_find_segment(self._h, _ptr(off, c_u32p), int(off.size) - 1, _ptr(x, c_u32p),
                                                     int(x.size), _ptr(out, c_u32p)))
        return out[:x.size]

    SPAN_RESULTS_32 = ("first_word", "words", "popcount", "all_set")
    SPAN_RESULTS_64 = ("first_mask", "last_mask", "word_view")

    def selftest_spans(self, bitmap, a, b, view=0):
        """catchhip_selftest_spans: what the helpers of csrc/spans.h returned for every interval [a[i], b[i]) over
        `bitmap` (uint64 words), by name; "word_view" is span_in_word for word `view`.  "painted" / "diff": all the
        intervals painted into one zeroed bitmap and marked on one zeroed difference array (64 * words + 1 entries)."""
        bm = np.ascontiguousarray(bitmap, dtype=np.uint64)
        a = np.ascontiguousarray(a, dtype=np.uint32)
        b = np.ascontiguousarray(b, dtype=np.uint32)
        if a.size != b.size:
            raise ValueError("selftest_spans: a and b must have one length")
        o32 = np.zeros((len(self.SPAN_RESULTS_32), a.size), dtype=np.uint32)
        o64 = np.zeros((len(self.SPAN_RESULTS_64), a.size), dtype=np.uint64)
        painted = np.zeros(bm.size, dtype=np.uint64)
        diff = np.zeros(64 * bm.size + 1, dtype=np.uint32)
        check(self._L.catchhip_selftest_spans(self._h, _ptr(bm, c_u64p), int(bm.size), _ptr(a, c_u32p), _ptr(b, c_u32p),
                                              int(a.size), int(view), _ptr(o32, c_u32p), _ptr(o64, c_u64p),
                                              _ptr(painted, c_u64p), _ptr(diff, c_u32p)))
        out = dict(zip(self.SPAN_RESULTS_32, o32))
        out.update(zip(self.SPAN_RESULTS_64, o64))
        out.update(painted=painted, diff=diff)
        return out

    # -- test entry point of the row build (tests/test_row_build.py) -------
    ROW_BUILDS = {"bucketed": 0, "radix": 1, "radix_if_overflow": 2}
    BK_NONE = 0xffffffff

    def selftest_row_build(self, hits, nb, form="scattered", hit_slots=None, wave_hits=None, bucket_set=None,
                           run_cnt=None, nruns=0, bounds=None, dedupe=False, want_sum=True, build="bucketed",
                           emit="host"):
        """catchhip_selftest_row_build: the row build's own functions on hit records filed the way a producer files
        them.  hits: (n, 4) uint32 {start, end, segment, bucket} in ARRIVAL order; a hit's rank is its arrival index
        inside its bucket.  form:
          "scattered"  record d = a work item; hit_slots (ascending slot numbers, one per hit; default 0..n-1) says
                       which work items hit, the others are misses (rank BK_NONE, record left as garbage);
          "compact"    the same with compact filing: wave_hits[w] hits stand at the front of slots 64 w ..;
          "grouped"    the records stand at bstart[bucket] + rank already; run_cnt (nb, stride) / nruns as the
                       key-grouped join leaves its anchor runs.
        Returns a dict: set / seg / start / end (the emitted table), mcnt / blmax / bsum per bucket, bstart, S (the
        grouped records after the merge, (hits, 4)), hits, rows, lmax, overflow, radix."""
        h = np.ascontiguousarray(hits, dtype=np.uint32).reshape(-1, 4)
        n, nb = h.shape[0], int(nb)
        bucket = h[:, 3].astype(np.int64)
        if n and int(bucket.max()) >= nb:
            raise ValueError("selftest_row_build: a hit names a bucket past nb")
        bcnt = np.bincount(bucket, minlength=nb).astype(np.uint32)
        bstart = np.zeros(nb + 1, dtype=np.uint32)
        np.cumsum(bcnt, out=bstart[1:])
        order = np.argsort(bucket, kind="stable")           # arrival order kept inside a bucket
        rank_of = np.zeros(n, dtype=np.uint32)
        rank_of[order] = (np.arange(n, dtype=np.int64) - bstart[bucket[order]].astype(np.int64)).astype(np.uint32)
        rec = rank = wcnt = d_bcnt = d_bstart = d_runs = None
        stride = 0
        if form == "grouped":
            rec = np.ascontiguousarray(h[order])
            d_bstart = bstart
            n_rec = n
            if run_cnt is not None:
                d_runs = np.ascontiguousarray(run_cnt, dtype=np.uint32).reshape(nb, -1)
                stride = d_runs.shape[1]
        else:
            if form == "compact":
                wave_hits = np.asarray(wave_hits, dtype=np.int64)
                if wave_hits.sum() != n or (wave_hits.size and (wave_hits.min() < 0 or wave_hits.max() > 64)):
                    raise ValueError("selftest_row_build: wave_hits must hold n hits, at most 64 per wave")
                first = np.repeat(64 * np.arange(wave_hits.size, dtype=np.int64) - (np.cumsum(wave_hits) - wave_hits),
                                  wave_hits)
                hit_slots = first + np.arange(n, dtype=np.int64)
                nslots = 64 * wave_hits.size
                wcnt = np.ascontiguousarray(np.append(wave_hits, 0), dtype=np.uint32)
            elif form == "scattered":
                hit_slots = np.arange(n, dtype=np.int64) if hit_slots is None else np.asarray(hit_slots, dtype=np.int64)
                if hit_slots.size != n or (n > 1 and (np.diff(hit_slots) <= 0).any()) or (n and hit_slots[0] < 0):
                    raise ValueError("selftest_row_build: hit_slots must be n ascending slot numbers")
                nslots = int(hit_slots[-1]) + 1 if n else 0
            else:
                raise ValueError("selftest_row_build: form %r" % (form,))
            # slots without a hit: a record that would do damage if anybody read it, and no rank
            rec = np.full((max(nslots, 1), 4), 0xdeadbeef, dtype=np.uint32)
            rank = np.full(max(nslots, 1), self.BK_NONE, dtype=np.uint32)
            rec[hit_slots] = h
            rank[hit_slots] = rank_of
            if form == "compact":                            # (compact filing never looks at the ranks past the hits)
                rank[np.setdiff1d(np.arange(nslots), hit_slots)] = 0
            d_bcnt = bcnt
            n_rec = nslots
        bs = None if bucket_set is None else np.ascontiguousarray(bucket_set, dtype=np.int32)
        if bs is not None and bs.size != nb:
            raise ValueError("selftest_row_build: bucket_set must have nb entries")
        bd = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.uint32)
        opt = np.array([int(bool(dedupe)), int(bool(want_sum)), self.ROW_BUILDS[build],
                        {"host": 0, "device": 1}[emit]], dtype=np.int32)
        cap = max(n, 1)
        o_set, o_seg = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        o_start, o_end = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        o_mcnt, o_blmax = np.zeros(nb, dtype=np.uint32), np.zeros(nb, dtype=np.uint32)
        o_bsum = np.zeros(nb, dtype=np.uint64)
        o_S = np.zeros((cap, 4), dtype=np.uint32)
        o_bstart = np.zeros(nb + 1, dtype=np.uint32)
        scalars = np.zeros(5, dtype=np.int64)

        def p(a, t):
            return None if a is None else _ptr(a, t)
        check(self._L.catchhip_selftest_row_build(
            self._h, p(rec, c_u32p), p(rank, c_u32p), p(wcnt, c_u32p), int(n_rec), p(d_bcnt, c_u32p),
            p(d_bstart, c_u32p), nb, p(bs, c_i32p), p(d_runs, c_u32p), int(stride), int(nruns), p(bd, c_u32p),
            0 if bd is None else int(bd.size) - 1, _ptr(opt, c_i32p), _ptr(o_set, c_i32p), _ptr(o_seg, c_i32p),
            _ptr(o_start, c_u32p), _ptr(o_end, c_u32p), _ptr(o_mcnt, c_u32p), _ptr(o_blmax, c_u32p),
            _ptr(o_bsum, c_u64p), _ptr(o_S, c_u32p), _ptr(o_bstart, c_u32p), _ptr(scalars, c_i64p)))
        rows = int(scalars[1])
        return {"set": o_set[:rows], "seg": o_seg[:rows], "start": o_start[:rows], "end": o_end[:rows],
                "mcnt": o_mcnt, "blmax": o_blmax, "bsum": o_bsum if want_sum else None, "bstart": o_bstart,
                "S": o_S[:n], "hits": int(scalars[0]), "rows": rows, "lmax": int(scalars[2]),
                "overflow": bool(scalars[3]), "radix": bool(scalars[4])}

    # -- test entry point of the seed table (tests/test_seed_table.py) -----
    def selftest_seed_table(self, probes, nent, mismatches, as_list=False, allow_filter=True):
        """catchhip_selftest_seed_table: the table of `probes`' anchor k-mers (nent anchor entries) as the key-grouped
        join builds it, or with as_list as the seed-list scan does.  Returns a dict: capacity, slots ((capacity, 4)
        uint32 {key lo, key hi, first, count}), ents (nent), present (the presence words; empty without the filter),
        bits_per_key, keys (slots with entries) and set_bits as the device counted them, entries (in the table),
        filtered, aslot (nent; only when filtered), anchors_per_probe."""
        nent = int(nent)
        room = 1024
        while room < 2 * nent:
            room *= 2
        slots = np.zeros((room, 4), dtype=np.uint32)
        ents = np.zeros(max(nent, 1), dtype=np.uint32)
        present = np.zeros(room // 8, dtype=np.uint32)
        aslot = np.zeros(max(nent, 1), dtype=np.uint32)
        scalars = np.zeros(8, dtype=np.int64)
        check(self._L.catchhip_selftest_seed_table(
            self._h, probes._h, int(mismatches), int(bool(as_list)), int(bool(allow_filter)), room,
            _ptr(slots, c_u32p), _ptr(ents, c_u32p), _ptr(present, c_u32p), _ptr(aslot, c_u32p), _ptr(scalars, c_i64p)))
        cap = int(scalars[0])
        filt = bool(scalars[6])
        return {"capacity": cap, "slots": slots[:cap], "ents": ents[:nent], "present": present[:int(scalars[3])],
                "bits_per_key": int(scalars[4]), "keys": int(scalars[1]), "set_bits": int(scalars[2]),
                "entries": int(scalars[5]), "filtered": filt, "aslot": aslot[:nent] if filt else None,
                "anchors_per_probe": int(scalars[7])}

    # -- near-duplicate filter --------------------------------------------
    def ndf_hamming(self, probe_strs, L, positions, dist_thres):
        n = len(probe_strs)
        buf, _ = _concat(probe_strs)
        pos = np.ascontiguousarray(positions, dtype=np.int32)
        ntables, k = pos.shape
        keep = np.zeros(max(n, 1), dtype=np.uint8)
        check(self._L.catchhip_ndf_hamming(self._h, _ptr(buf, c_u8p), n, L,
                                           _ptr(pos, c_i32p), ntables, k,
                                           dist_thres, _ptr(keep, c_u8p)))
        return keep[:n].astype(bool)


    def ndf_minhash(self, probe_strs, kmer_size, params, dist_thres):
        """catchhip_ndf_minhash; params[table][fn] = (a, b)."""
        n = len(probe_strs)
        buf, off = _concat(probe_strs)
        ab = np.ascontiguousarray(params, dtype=np.int64)
        ntables, k = ab.shape[0], ab.shape[1]
        keep = np.zeros(max(n, 1), dtype=np.uint8)
        check(self._L.catchhip_ndf_minhash(
            self._h, _ptr(buf, c_u8p), _ptr(off, c_i64p), n, int(kmer_size),
            _ptr(ab, c_i64p), ntables, k, float(dist_thres), _ptr(keep, c_u8p)))
        return keep[:n].astype(bool)


    def ndf_minhash_many(self, groups, kmer_size, params, dist_thres):
        """catchhip_ndf_minhash_many; groups = lists of probe strings,
        params[group][table][fn] = (a, b).  Returns one bool array per group."""
        flat = [s for g in groups for s in g]
        n = len(flat)
        if n == 0:
            return [np.zeros(0, dtype=bool) for _ in groups]
        buf, off = _concat(flat)
        goff = np.zeros(len(groups) + 1, dtype=np.int64)
        np.cumsum([len(g) for g in groups], out=goff[1:])
        ab = np.ascontiguousarray(params, dtype=np.int64)
        assert ab.ndim == 4 and ab.shape[0] == len(groups)
        ntables, k = ab.shape[1], ab.shape[2]
        keep = np.zeros(n, dtype=np.uint8)
        check(self._L.catchhip_ndf_minhash_many(
            self._h, _ptr(buf, c_u8p), _ptr(off, c_i64p), n, _ptr(goff, c_i64p),
            len(groups), int(kmer_size), _ptr(ab, c_i64p), ntables, k,
            float(dist_thres), _ptr(keep, c_u8p)))
        keep = keep.astype(bool)
        return [keep[goff[g]:goff[g + 1]] for g in range(len(groups))]


class Targets:
    """Device-resident target sequences (catchhip_targets).
    genomes: list of genomes, each a list of sequence strings."""

    def __init__(self, ctx, genomes):
        self.ctx = ctx
        if isinstance(genomes, FragmentTable):       # every fragment a genome of one sequence
            seqs, sgn = genomes, np.arange(len(genomes), dtype=np.int32)
        else:
            seqs, sg = [], []
            for j, g in enumerate(genomes):
                for s in g:
                    seqs.append(s)
                    sg.append(j)
            sgn = np.asarray(sg, dtype=np.int32)
        if sgn.size == 0:
            sgn = np.zeros(1, dtype=np.int32)
        self.nseq = len(seqs)
        self.ngenomes = len(genomes)
        self._h = ctypes.c_void_p()
        ptrs = _str_pointers(seqs) if len(seqs) else None
        if ptrs is not None:
            # one pointer per sequence: the library gathers them into pinned
            # memory itself (no 600 MB join + encode on the Python side)
            parr, lens = ptrs
            off = np.zeros(len(seqs) + 1, dtype=np.int64)
            np.cumsum(lens, out=off[1:])
            check(ctx._L.catchhip_targets_create_ptrs(
                ctx._h, parr, _ptr(lens, c_i64p), _ptr(sgn, c_i32p), self.nseq,
                self.ngenomes, ctypes.byref(self._h)))
        else:
            buf, off = _concat(seqs)
            check(ctx._L.catchhip_targets_create(
                ctx._h, _ptr(buf, c_u8p), _ptr(off, c_i64p), _ptr(sgn, c_i32p),
                self.nseq, self.ngenomes, ctypes.byref(self._h)))
        self.total = int(off[-1])
        self.seq_off = off      # global start of every sequence (+ total)

    def rebind(self, ctx):
        """catchhip_targets_rebind: hand the object to another context of the
        same device (waits for the stream it was built on)."""
        check(ctx._L.catchhip_targets_rebind(self._h, ctx._h))
        self.ctx = ctx
        return self

    def set_groups(self, group_of_genome):
        """catchhip_targets_set_groups (one entry per genome)."""
        g = np.ascontiguousarray(group_of_genome, dtype=np.int32)
        assert g.size == self.ngenomes
        if g.size == 0:
            g = np.zeros(1, dtype=np.int32)
        check(self.ctx._L.catchhip_targets_set_groups(self.ctx._h, self._h,
                                                      _ptr(g, c_i32p)))

    def close(self):
        if self._h and self.ctx._h:      # (see Context.close)
            self.ctx._L.catchhip_targets_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Probes:
    """Device-resident unique probes + anchor table (catchhip_probes)."""

    def __init__(self, ctx, uniq, owner, ent_probe, ent_pos, k):
        self.ctx = ctx
        self.n = len(uniq)
        buf, off = _concat(uniq)
        owner = np.ascontiguousarray(owner, dtype=np.int32)
        ep = np.ascontiguousarray(ent_probe, dtype=np.int32)
        eo = np.ascontiguousarray(ent_pos, dtype=np.int32)
        if owner.size == 0:
            owner = np.zeros(1, dtype=np.int32)
        nent = int(ep.size) if self.n else 0
        if ep.size == 0:
            ep = np.zeros(1, dtype=np.int32)
            eo = np.zeros(1, dtype=np.int32)
        self._h = ctypes.c_void_p()
        check(ctx._L.catchhip_probes_create(
            ctx._h, _ptr(buf, c_u8p), _ptr(off, c_i64p), self.n,
            _ptr(owner, c_i32p), _ptr(ep, c_i32p), _ptr(eo, c_i32p), nent,
            int(k or 0), ctypes.byref(self._h)))

    def rebind(self, ctx):
        """catchhip_probes_rebind (see Targets.rebind)."""
        check(ctx._L.catchhip_probes_rebind(self._h, ctx._h))
        self.ctx = ctx
        return self

    def set_groups(self, group_of_probe):
        """catchhip_probes_set_groups (one entry per unique probe)."""
        g = np.ascontiguousarray(group_of_probe, dtype=np.int32)
        assert g.size == self.n
        if g.size == 0:
            g = np.zeros(1, dtype=np.int32)
        check(self.ctx._L.catchhip_probes_set_groups(self.ctx._h, self._h,
                                                     _ptr(g, c_i32p)))

    def close(self):
        if self._h and self.ctx._h:      # (see Context.close)
            self.ctx._L.catchhip_probes_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KmerIndex:
    """The k-mers of a background on the device (catchhip_kmer_index, not in
    the reference): the sorted distinct canonical codes of every valid k-mer of
    `seqs` (strings; only A, C, G, T are bases, no k-mer spans two of them) and
    a prefix directory, for Candidates.drop_background.  Built on ctx, usable
    from every context of ctx's device, and it outlives ctx.  n_valid: valid
    k-mer positions; n_unique: distinct canonical codes.  mismatches = M > 0
    (catchhip_kmer_index_create_tolerant, k >= 8 (M + 1), M <= 2) makes the
    index tolerant: M + 1 views of the codes, and drop_background and measure
    then count k-mers within M mismatches of the background."""

    def __init__(self, ctx, seqs, k, mismatches=0):
        self.ctx, self.device, self.k, self.mismatches = ctx, ctx.device, int(k), int(mismatches)
        self._L = ctx._L
        self._h = ctypes.c_void_p()
        seqs = list(seqs)
        buf, off = _concat(seqs)
        nv, nu = ctypes.c_int64(0), ctypes.c_int64(0)
        if self.mismatches == 0:
            check(self._L.catchhip_kmer_index_create(
                ctx._h, _ptr(buf, c_u8p), _ptr(off, c_i64p), len(seqs), self.k,
                ctypes.byref(self._h), ctypes.byref(nv), ctypes.byref(nu)))
        else:
            check(self._L.catchhip_kmer_index_create_tolerant(
                ctx._h, _ptr(buf, c_u8p), _ptr(off, c_i64p), len(seqs), self.k, self.mismatches,
                ctypes.byref(self._h), ctypes.byref(nv), ctypes.byref(nu)))
        self.n_valid, self.n_unique = nv.value, nu.value

    def fetch(self, ctx=None):
        """The sorted distinct canonical codes (uint64), through any context of
        the device (default: the one it was built on)."""
        out = np.zeros(max(self.n_unique, 1), dtype=np.uint64)
        check(self._L.catchhip_kmer_index_fetch((ctx or self.ctx)._h, self._h, _ptr(out, c_u64p)))
        return out[:self.n_unique]

    def fetch_view(self, b, ctx=None):
        """The sorted codes of view b = 0 .. mismatches (uint64): every code
        rotated left by 2 * floor(b k / (mismatches + 1)) bits inside its 2k."""
        out = np.zeros(max(self.n_unique, 1), dtype=np.uint64)
        check(self._L.catchhip_kmer_index_fetch_view((ctx or self.ctx)._h, self._h, int(b), _ptr(out, c_u64p)))
        return out[:self.n_unique]

    def close(self):
        if self._h:
            self._L.catchhip_kmer_index_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Candidates:
    """Unique candidate probes of a Targets object, on the device
    (catchhip_candidates): sliding windows + exact de-duplication."""

    def __init__(self, ctx, targets, probe_length, probe_stride,
                 seq_length_to_skip=None):
        self.ctx = ctx
        self.targets = targets          # keeps the targets alive
        self.L = int(probe_length)
        self._h = ctypes.c_void_p()
        nc, nu = ctypes.c_int64(0), ctypes.c_int64(0)
        check(ctx._L.catchhip_candidates_create(
            ctx._h, targets._h, self.L, int(probe_stride),
            -1 if seq_length_to_skip is None else int(seq_length_to_skip),
            ctypes.byref(self._h), ctypes.byref(nc), ctypes.byref(nu)))
        self.ncandidates, self.n = nc.value, nu.value

    def rebind(self, ctx):
        """catchhip_candidates_rebind (see Targets.rebind)."""
        check(ctx._L.catchhip_candidates_rebind(self._h, ctx._h))
        self.ctx = ctx
        return self

    def positions(self, ids=None):
        """Global start (concatenated target coordinate) of unique candidates
        `ids` (default: all)."""
        if ids is None:
            n, idp = self.n, None
        else:
            ids = np.ascontiguousarray(ids, dtype=np.int64)
            n, idp = int(ids.size), _ptr(ids, c_i64p)
        out = np.zeros(max(n, 1), dtype=np.int64)
        check(self.ctx._L.catchhip_candidates_fetch(
            self.ctx._h, self._h, idp, n, _ptr(out, c_i64p)))
        return out[:n]

    def drop_polya(self, length, mismatches, min_exact=6):
        """catchhip_candidates_drop_polya: the unique candidates without those
        the poly(A) filter drops, order, multiplicities and groups kept."""
        nk = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_candidates_drop_polya(
            self.ctx._h, self._h, int(length), int(mismatches), int(min_exact),
            ctypes.byref(nk)))
        self.n = nk.value

    def drop_composition(self, gc_lo=-1, gc_hi=-1, max_run=-1, dust_x10=-1, dust_window=64):
        """catchhip_candidates_drop_composition (not in the reference): the
        unique candidates without those a composition rule drops (GC count
        outside gc_lo..gc_hi, a homopolymer run above max_run, a window of
        dust_window bytes scoring above dust_x10; -1: rule off), order,
        multiplicities and groups kept.  Returns the candidates dropped, with
        multiplicity: [GC, homopolymer, low complexity, any rule]."""
        nk = ctypes.c_int64(0)
        dropped = np.zeros(4, dtype=np.int64)
        check(self.ctx._L.catchhip_candidates_drop_composition(
            self.ctx._h, self._h, int(gc_lo), int(gc_hi), int(max_run), int(dust_x10),
            int(dust_window), _ptr(dropped, c_i64p), ctypes.byref(nk)))
        self.n = nk.value
        return [int(x) for x in dropped]

    def drop_structure(self, max_stem=-1, min_loop=3, max_dimer=-1):
        """catchhip_candidates_drop_structure (not in the reference): the
        unique candidates without those a secondary-structure rule drops (a
        hairpin stem of more than max_stem base pairs around a loop of at
        least min_loop characters, a self-dimer of more than max_dimer
        consecutive base pairs; -1: rule off), order, multiplicities and groups
        kept.  Returns the candidates dropped, with multiplicity: [hairpin,
        self-dimer, any rule]."""
        nk = ctypes.c_int64(0)
        dropped = np.zeros(3, dtype=np.int64)
        check(self.ctx._L.catchhip_candidates_drop_structure(
            self.ctx._h, self._h, int(max_stem), int(min_loop), int(max_dimer),
            _ptr(dropped, c_i64p), ctypes.byref(nk)))
        self.n = nk.value
        return [int(x) for x in dropped]

    def drop_tm(self, q, offset_c, lo_c=None, hi_c=None, histogram=True):
        """catchhip_candidates_drop_tm (not in the reference): the nearest-
        neighbour melting temperature tm_c of every unique candidate
        (catch_amd/filter/tm_filter.py has the rule; q = Q(L), offset_c =
        27315 + f).  With lo_c and hi_c the candidates outside lo_c..hi_c are
        dropped, order, multiplicities and groups kept; without them the list
        is untouched.  Returns ([below, above, any] dropped, with multiplicity,
        the 128 bins of whole degrees over the candidates the call saw, with
        multiplicity -- None if histogram is false)."""
        if (lo_c is None) != (hi_c is None):
            raise ValueError("drop_tm: lo_c and hi_c go together")
        nk = ctypes.c_int64(0)
        dropped = np.zeros(3, dtype=np.int64)
        hist = np.zeros(128, dtype=np.uint64) if histogram else None
        check(self.ctx._L.catchhip_candidates_drop_tm(
            self.ctx._h, self._h, int(q), int(offset_c), 0 if lo_c is None else 1,
            0 if lo_c is None else int(lo_c), 0 if hi_c is None else int(hi_c),
            _ptr(dropped, c_i64p), None if hist is None else _ptr(hist, c_u64p), ctypes.byref(nk)))
        self.n = nk.value
        return [int(x) for x in dropped], None if hist is None else [int(x) for x in hist]

    def drop_background(self, index, max_hits=None, histogram=True):
        """catchhip_candidates_drop_background (not in the reference): the
        number of k-mers every unique candidate shares with the background
        behind `index` (a KmerIndex of this device; catch_amd/filter/
        background_filter.py has the rule), within index.mismatches
        substitutions.  With max_hits the candidates with
        more hits are dropped, order, multiplicities and groups kept; without
        it the list is untouched.  Returns (candidates dropped, with
        multiplicity, the 256 bins of min(hits, 255) over the candidates the
        call saw, with multiplicity -- None if histogram is false)."""
        nk = ctypes.c_int64(0)
        dropped = np.zeros(1, dtype=np.int64)
        hist = np.zeros(256, dtype=np.uint64) if histogram else None
        check(self.ctx._L.catchhip_candidates_drop_background(
            self.ctx._h, self._h, index._h, 0 if max_hits is None else 1,
            0 if max_hits is None else int(max_hits), _ptr(dropped, c_i64p),
            None if hist is None else _ptr(hist, c_u64p), ctypes.byref(nk)))
        self.n = nk.value
        return int(dropped[0]), None if hist is None else [int(x) for x in hist]

    MEASURE_FAMILIES = {"composition": (1, ("gc", "homopolymer", "dust")), "structure": (2, ("stem", "dimer")),
                        "tm": (4, ("tm_c",)), "hits": (8, ("hits",))}

    def measure(self, what=("composition", "structure"), min_loop=3, dust_window=64, tm=None, index=None,
                values=False, histograms=True):
        """catchhip_candidates_measure (not in the reference): the value behind
        every rule, for every unique candidate (catch_amd/filter/quality.py has
        the definitions); the list is left exactly as it was.  what: the
        families to compute, of "composition" (gc, homopolymer, dust),
        "structure" (stem, dimer), "tm" (tm_c; tm = (q, offset_c) as for
        drop_tm) and "hits" (index = a KmerIndex of this device); none is
        valid.  Returns a dict: with values, a NumPy array per quantity of the
        families asked for (uint16; tm_c int32, None where the candidates have
        fewer than 2 characters; hits uint32); with histograms, under
        "histograms", {quantity: 1,280 bins of min(value, 1279), with
        multiplicity} for the quantities of "composition" and "structure"."""
        if isinstance(what, str):
            what = (what,)
        what = list(what)
        for w in what:
            if w not in self.MEASURE_FAMILIES:
                raise ValueError("measure: unknown family %r (one of %s)" % (w, ", ".join(self.MEASURE_FAMILIES)))
        if "tm" in what and tm is None:
            raise ValueError("measure: \"tm\" needs tm = (q, offset_c)")
        if "hits" in what and index is None:
            raise ValueError("measure: \"hits\" needs an index")
        mask = 0
        for w in what:
            mask |= self.MEASURE_FAMILIES[w][0]
        n = max(self.n, 1)
        arrays = {}
        if values:
            for w in what:
                for name in self.MEASURE_FAMILIES[w][1]:
                    arrays[name] = np.zeros(n, dtype={"tm_c": np.int32, "hits": np.uint32}.get(name, np.uint16))
        hist = np.zeros(5 * 1280, dtype=np.uint64) if histograms else None
        q, offset_c = (0, 0) if "tm" not in what else (int(tm[0]), int(tm[1]))

        def p(name, t):
            return _ptr(arrays[name], t) if name in arrays else None
        check(self.ctx._L.catchhip_candidates_measure(
            self.ctx._h, self._h, mask, int(min_loop), int(dust_window), q, offset_c,
            index._h if "hits" in what else None, 1 if values else 0,
            p("gc", c_u16p), p("homopolymer", c_u16p), p("dust", c_u16p), p("stem", c_u16p), p("dimer", c_u16p),
            p("tm_c", c_i32p), p("hits", c_u32p), None if hist is None else _ptr(hist, c_u64p)))
        out = {name: a[:self.n] for name, a in arrays.items()}
        if "tm_c" in out and self.L < 2:
            out["tm_c"] = None
        if histograms:
            names = ("gc", "homopolymer", "dust", "stem", "dimer")
            asked = [name for w in what for name in self.MEASURE_FAMILIES[w][1]]
            out["histograms"] = {name: hist[1280 * k:1280 * (k + 1)].astype(np.int64)
                                 for k, name in enumerate(names) if name in asked}
        return out

    def multiplicities(self):
        """How many candidates equal every unique one (before a near-duplicate filter)."""
        out = np.zeros(max(self.n, 1), dtype=np.uint32)
        check(self.ctx._L.catchhip_candidates_multiplicities(
            self.ctx._h, self._h, _ptr(out, c_u32p)))
        return out[:self.n]

    def ndf_hamming(self, positions, dist_thres):
        """catchhip_candidates_ndf_hamming: the list becomes the candidates the
        Hamming near-duplicate filter keeps, in its priority order."""
        pos = np.ascontiguousarray(positions, dtype=np.int32)
        nk = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_candidates_ndf_hamming(
            self.ctx._h, self._h, _ptr(pos, c_i32p), pos.shape[0], pos.shape[1],
            int(dist_thres), ctypes.byref(nk)))
        self.n = nk.value

    def ndf_minhash(self, kmer_size, params, dist_thres):
        """catchhip_candidates_ndf_minhash; params[table][fn] = (a, b)."""
        ab = np.ascontiguousarray(params, dtype=np.int64)
        nk = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_candidates_ndf_minhash(
            self.ctx._h, self._h, int(kmer_size), _ptr(ab, c_i64p), ab.shape[0],
            ab.shape[1], float(dist_thres), ctypes.byref(nk)))
        self.n = nk.value

    def ndf_hamming_many(self, positions, dist_thres):
        """catchhip_candidates_ndf_hamming_many (grouped targets);
        positions[group][table][j]."""
        pos = np.ascontiguousarray(positions, dtype=np.int32)
        assert pos.ndim == 3
        nk = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_candidates_ndf_hamming_many(
            self.ctx._h, self._h, _ptr(pos, c_i32p), pos.shape[0], pos.shape[1],
            pos.shape[2], int(dist_thres), ctypes.byref(nk)))
        self.n = nk.value

    def ndf_minhash_many(self, kmer_size, params, dist_thres):
        """catchhip_candidates_ndf_minhash_many (grouped targets);
        params[group][table][fn] = (a, b)."""
        ab = np.ascontiguousarray(params, dtype=np.int64)
        assert ab.ndim == 4
        nk = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_candidates_ndf_minhash_many(
            self.ctx._h, self._h, int(kmer_size), _ptr(ab, c_i64p), ab.shape[0],
            ab.shape[1], ab.shape[2], float(dist_thres), ctypes.byref(nk)))
        self.n = nk.value

    def groups(self):
        """Group of every unique candidate (zeros without grouped targets)."""
        out = np.zeros(max(self.n, 1), dtype=np.int32)
        check(self.ctx._L.catchhip_candidates_groups(self.ctx._h, self._h,
                                                     _ptr(out, c_i32p)))
        return out[:self.n]

    def probes(self, k, ent_probe=None, ent_pos=None):
        """Probes object of the unique candidates; anchors given (sorted by
        (probe, position), unique) or the pigeonhole table when omitted."""
        p = Probes.__new__(Probes)
        p.ctx, p.n = self.ctx, self.n
        p._h = ctypes.c_void_p()
        if ent_probe is None:
            check(self.ctx._L.catchhip_probes_from_candidates(
                self.ctx._h, self._h, None, None, 0, int(k), ctypes.byref(p._h)))
        else:
            ep = np.ascontiguousarray(ent_probe, dtype=np.int32)
            eo = np.ascontiguousarray(ent_pos, dtype=np.int32)
            nent = int(ep.size)
            if nent == 0:
                ep = np.zeros(1, np.int32)
                eo = np.zeros(1, np.int32)
            check(self.ctx._L.catchhip_probes_from_candidates(
                self.ctx._h, self._h, _ptr(ep, c_i32p), _ptr(eo, c_i32p), nent,
                int(k), ctypes.byref(p._h)))
        return p

    def probes_from_draws(self, k, draws):
        """Probes object of the unique candidates with random anchors given as
        the positions np.random drew (uint8 [n][draws per probe]): the sorted
        distinct positions of every probe, built on the device."""
        p = Probes.__new__(Probes)
        p.ctx, p.n = self.ctx, self.n
        p._h = ctypes.c_void_p()
        d = np.ascontiguousarray(draws, dtype=np.uint8)
        if self.n == 0:
            d = np.zeros((1, 1), np.uint8)
        assert d.ndim == 2 and (self.n == 0 or d.shape[0] == self.n)
        check(self.ctx._L.catchhip_probes_from_candidates_draws(
            self.ctx._h, self._h, _ptr(d, c_u8p), int(d.shape[1]), int(k), ctypes.byref(p._h)))
        return p

    def close(self):
        if self._h and self.ctx._h:      # (see Context.close)
            self.ctx._L.catchhip_candidates_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Rows:
    """Device-resident cover rows (catchhip_rows)."""

    def __init__(self, ctx, handle, n, ngenomes=None):
        self.ctx = ctx
        self._h = handle
        self.n = int(n)
        self.ngenomes = ngenomes      # universes of the coordinate space (None: the maker did not say)
        self.last_prune_rounds = 0    # rounds the device took in the last prune() of these rows
        self.last_gains_ms = 0.0      # device time and launches of the last pick_gains() of these rows, summed over
        self.last_gains_launches = 0  # the library calls it was split into
        self.last_uncovered_ms = 0.0  # device time and launches of the last uncovered() of these rows
        self.last_uncovered_launches = 0

    @staticmethod
    def scan(ctx, probes, targets, mismatches, lcf_thres, island=0,
             cover_extension=0, mode=SCAN_AUTO, merge=True):
        """catchhip_cover_scan, or with merge=False catchhip_cover_ranges
        (every distinct cover range of every probe, nothing merged)."""
        h = ctypes.c_void_p()
        n = ctypes.c_int64(0)
        fn = ctx._L.catchhip_cover_scan if merge else ctx._L.catchhip_cover_ranges
        check(fn(
            ctx._h, probes._h, targets._h, int(mismatches), int(lcf_thres),
            int(island), int(cover_extension), int(mode), ctypes.byref(h),
            ctypes.byref(n)))
        return Rows(ctx, h, n.value, getattr(targets, "ngenomes", None))

    @staticmethod
    def scan_first_seen(ctx, probes, targets, mismatches, lcf_thres, island=0,
                        cover_extension=0, mode=SCAN_AUTO, anchor_order=None):
        """catchhip_cover_scan_first_seen: merged rows that also carry, per
        (set, universe) group, the key of the first accepted seed
        (fetch_first_seen)."""
        h = ctypes.c_void_p()
        n = ctypes.c_int64(0)
        order = (None if anchor_order is None
                 else np.ascontiguousarray(anchor_order, dtype=np.uint32))
        check(ctx._L.catchhip_cover_scan_first_seen(
            ctx._h, probes._h, targets._h, int(mismatches), int(lcf_thres),
            int(island), int(cover_extension), int(mode),
            None if order is None else _ptr(order, c_u32p),
            ctypes.byref(h), ctypes.byref(n)))
        return Rows(ctx, h, n.value, getattr(targets, "ngenomes", None))

    def adapter_votes(self, multiplicity):
        """catchhip_adapter_votes -> (A votes, B votes) per set id."""
        mult = np.ascontiguousarray(multiplicity, dtype=np.int64)
        n = int(mult.size)
        a = np.zeros(max(n, 1), dtype=np.int64)
        b = np.zeros(max(n, 1), dtype=np.int64)
        check(self.ctx._L.catchhip_adapter_votes(
            self.ctx._h, self._h, n, _ptr(mult, c_i64p), _ptr(a, c_i64p),
            _ptr(b, c_i64p)))
        return a[:n], b[:n]

    def stats(self, ngenomes, num_sets=0):
        """catchhip_rows_stats -> (total_len[ngenomes], union_len[ngenomes],
        universes_per_set[num_sets])."""
        tl = np.zeros(max(ngenomes, 1), dtype=np.int64)
        ul = np.zeros(max(ngenomes, 1), dtype=np.int64)
        ps = np.zeros(max(num_sets, 1), dtype=np.int64)
        check(self.ctx._L.catchhip_rows_stats(
            self.ctx._h, self._h, _ptr(tl, c_i64p), _ptr(ul, c_i64p),
            int(num_sets), _ptr(ps, c_i64p)))
        return tl[:ngenomes], ul[:ngenomes], ps[:num_sets]

    def first_seen_per_set(self, num_sets):
        """catchhip_rows_first_seen_per_set -> (first universe int32[num_sets] (-1: no rows), its first-seen
        key uint64[num_sets]); rows from scan_first_seen."""
        num_sets = int(num_sets)
        un = np.full(max(num_sets, 1), -1, dtype=np.int32)
        key = np.zeros(max(num_sets, 1), dtype=np.uint64)
        check(self.ctx._L.catchhip_rows_first_seen_per_set(
            self.ctx._h, self._h, num_sets, _ptr(un, c_i32p), _ptr(key, c_u64p)))
        return un[:num_sets], key[:num_sets]

    def window_depth(self, span_first, window_length, window_stride):
        """catchhip_rows_window_depth: span s = universes [span_first[s], span_first[s + 1]) ->
        (sums uint64[nwin], counts uint32[nwin], win_off int64[nspans + 1]): per window, in span order, the
        sum of the 16-bit depth over its bases and their number; windows of span s are win_off[s]:win_off[s + 1]."""
        sf = np.ascontiguousarray(span_first, dtype=np.int64)
        nspans = max(int(sf.size) - 1, 0)
        per_span = np.zeros(max(nspans, 1), dtype=np.int64)
        fn = self.ctx._L.catchhip_rows_window_depth
        check(fn(self.ctx._h, self._h, _ptr(sf, c_i64p) if sf.size else None, nspans, int(window_length),
                 int(window_stride), _ptr(per_span, c_i64p), None, None, 0))
        win_off = np.zeros(nspans + 1, dtype=np.int64)
        np.cumsum(per_span[:nspans], out=win_off[1:])
        nwin = int(win_off[-1])
        sums = np.zeros(max(nwin, 1), dtype=np.uint64)
        counts = np.zeros(max(nwin, 1), dtype=np.uint32)
        check(fn(self.ctx._h, self._h, _ptr(sf, c_i64p) if sf.size else None, nspans, int(window_length),
                 int(window_stride), _ptr(per_span, c_i64p), _ptr(sums, c_u64p), _ptr(counts, c_u32p), nwin))
        return sums[:nwin], counts[:nwin], win_off

    def uncovered(self, targets=None, min_depth=1, min_length=1, min_unambig=1, mask=None):
        """catchhip_rows_uncovered (mask, a BaseMask over these universes: catchhip_rows_uncovered_within, the runs
        of WANTED bases -- an unwanted base ends a run as a covered one does)
        -> (universe int32[n], start int64[n], end int64[n], unambig int64[n],
        per_universe int64[ngenomes, 3]): the maximal runs of bases, inside one universe, that fewer than
        `min_depth` rows cover, in (universe, start) order, start and end local to the universe; reported are the
        runs of `min_length` bases and more of which at least `min_unambig` are A, C, G or T in `targets` (Targets
        with one genome per sequence over these universes; None: every base counts).  per_universe[u] = (regions,
        bases, longest) over the reported runs of universe u.  The device time and the launches are left in
        `last_uncovered_ms` / `last_uncovered_launches`."""
        if self.ngenomes is None:
            raise ValueError("uncovered: rows of an unknown number of universes")
        ng = int(self.ngenomes)
        per = np.zeros((max(ng, 1), 3), dtype=np.int64)
        h = ctypes.c_void_p()
        n = ctypes.c_int64(0)
        th = None if targets is None else targets._h
        if mask is None:
            check(self.ctx._L.catchhip_rows_uncovered(
                self.ctx._h, self._h, th, int(min_depth), int(min_length),
                int(min_unambig), ctypes.byref(h), ctypes.byref(n), _ptr(per, c_i64p)))
        else:
            check(self.ctx._L.catchhip_rows_uncovered_within(
                self.ctx._h, self._h, th, mask._h, int(min_depth), int(min_length),
                int(min_unambig), ctypes.byref(h), ctypes.byref(n), _ptr(per, c_i64p)))
        self.last_uncovered_ms, self.last_uncovered_launches = self.ctx.kernel_ms(PHASE_ROWS)
        regions = Rows(self.ctx, h, n.value, ng)
        try:
            ua, un, st, en = regions.fetch()
        finally:
            regions.close()
        # (the count travels in the 32 bits of the set id column)
        return un, st, en, ua.view(np.uint32).astype(np.int64), per[:ng]

    def cover_check(self, num_sets, picks, universe_p=None):
        """catchhip_rows_cover_check: replays `picks` (set ids in pick order) over these rows with kernels that
        share nothing with the solvers -> dict(picks_without_gain, universes_short, bad_pick_ids, universe_bases,
        covered_bases); a correct solution has the first three at zero."""
        pk = np.ascontiguousarray(picks, dtype=np.int64)
        up = None if universe_p is None else np.ascontiguousarray(universe_p, dtype=np.float64)
        out = np.zeros(5, dtype=np.int64)
        check(self.ctx._L.catchhip_rows_cover_check(
            self.ctx._h, self._h, int(num_sets), _ptr(pk, c_i64p) if pk.size else None, int(pk.size),
            None if up is None else _ptr(up, c_f64p), _ptr(out, c_i64p)))
        return dict(picks_without_gain=int(out[0]), universes_short=int(out[1]), bad_pick_ids=int(out[2]),
                    universe_bases=int(out[3]), covered_bases=int(out[4]))

    def fetch_first_seen(self):
        """uint64[n]: (k-mer position in the universe << 32) | anchor order."""
        out = np.zeros(max(self.n, 1), dtype=np.uint64)
        check(self.ctx._L.catchhip_rows_fetch_first_seen(
            self.ctx._h, self._h, _ptr(out, c_u64p)))
        return out[:self.n]

    @staticmethod
    def from_host(ctx, set_id, universe, start, end, genome_len):
        si = np.ascontiguousarray(set_id, dtype=np.int32)
        un = np.ascontiguousarray(universe, dtype=np.int32)
        st = np.ascontiguousarray(start, dtype=np.int64)
        en = np.ascontiguousarray(end, dtype=np.int64)
        gl = np.ascontiguousarray(genome_len, dtype=np.int64)
        n = int(si.size)
        ng = int(gl.size)
        if n == 0:
            si = np.zeros(1, np.int32); un = np.zeros(1, np.int32)
            st = np.zeros(1, np.int64); en = np.zeros(1, np.int64)
        if ng == 0:
            gl = np.zeros(1, np.int64)
        h = ctypes.c_void_p()
        check(ctx._L.catchhip_rows_from_host(
            ctx._h, _ptr(si, c_i32p), _ptr(un, c_i32p), _ptr(st, c_i64p),
            _ptr(en, c_i64p), n, _ptr(gl, c_i64p), ng, ctypes.byref(h)))
        return Rows(ctx, h, n, int(np.asarray(genome_len).size))

    def extend(self, targets, cover_extensions):
        """catchhip_rows_extend: these rows (a cover scan at cover_extension 0)
        at every extension given -> one Rows per extension, equal to a scan of
        the same probes and targets at that extension."""
        ext = np.ascontiguousarray(cover_extensions, dtype=np.int32)
        n = int(ext.size)
        hs = (ctypes.c_void_p * max(n, 1))()
        nr = np.zeros(max(n, 1), dtype=np.int64)
        check(self.ctx._L.catchhip_rows_extend(
            self.ctx._h, self._h, targets._h, n,
            _ptr(ext, c_i32p) if n else None, hs, _ptr(nr, c_i64p)))
        return [Rows(self.ctx, ctypes.c_void_p(hs[i]), nr[i], self.ngenomes) for i in range(n)]

    def subtract(self, covered):
        """catchhip_rows_subtract: these rows without the bases that `covered`
        (Rows over the same universes, any set ids) covers -- every row cut
        into its uncovered runs, set, universe and order kept."""
        h = ctypes.c_void_p()
        n = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_rows_subtract(
            self.ctx._h, self._h, covered._h, ctypes.byref(h), ctypes.byref(n)))
        return Rows(self.ctx, h, n.value, self.ngenomes)

    def union(self, other):
        """catchhip_rows_union: per (set, universe) the union of these rows and
        `other`'s (Rows in the solver's form over the same universes, any set
        ids), rows that overlap or touch merged -- sorted by (set, universe,
        start), ready for greedy()."""
        h = ctypes.c_void_p()
        n = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_rows_union(
            self.ctx._h, self._h, other._h, ctypes.byref(h), ctypes.byref(n)))
        return Rows(self.ctx, h, n.value, self.ngenomes)

    def longest(self):
        """catchhip_rows_longest: the length of the longest row, as the table
        holds it for the solvers."""
        out = ctypes.c_uint32(0)
        check(self.ctx._L.catchhip_rows_longest(self._h, ctypes.byref(out)))
        return int(out.value)

    def restrict(self, mask):
        """catchhip_rows_restrict: these rows cut to their maximal runs of the
        bases `mask` (a BaseMask over the same universes) wants -- set, universe
        and order kept."""
        h = ctypes.c_void_p()
        n = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_rows_restrict(
            self.ctx._h, self._h, mask._h, ctypes.byref(h), ctypes.byref(n)))
        return Rows(self.ctx, h, n.value, self.ngenomes)

    def below_depth(self, num_sets, picks, depth):
        """catchhip_rows_below_depth -> (Rows, reached int64[ngenomes]): the rows
        of the sets not in `picks`, cut into their runs of bases that fewer than
        `depth` picked sets cover; reached[u] = the bases of universe u that
        `depth` or more of them cover."""
        if self.ngenomes is None:
            raise ValueError("below_depth: rows of an unknown number of universes")
        pk = np.ascontiguousarray(picks, dtype=np.int64)
        ng = int(self.ngenomes)
        reached = np.zeros(max(ng, 1), dtype=np.int64)
        h = ctypes.c_void_p()
        n = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_rows_below_depth(
            self.ctx._h, self._h, int(num_sets), _ptr(pk, c_i64p) if pk.size else None,
            int(pk.size), int(depth), ctypes.byref(h), ctypes.byref(n), _ptr(reached, c_i64p)))
        return Rows(self.ctx, h, n.value, ng), reached[:ng]

    def drop_sets(self, num_sets, drop):
        """catchhip_rows_drop_sets: these rows without those of the sets s with
        drop[s] set (one flag per set id, num_sets of them) -- order and set ids
        kept, ready for greedy(), subtract() and below_depth()."""
        num_sets = int(num_sets)
        flags = np.ascontiguousarray(np.asarray(drop) != 0, dtype=np.uint8)
        if flags.ndim != 1 or flags.size != num_sets:
            raise ValueError("drop_sets: %d flags for %d sets" % (flags.size, num_sets))
        if num_sets == 0:
            flags = np.zeros(1, dtype=np.uint8)
        h = ctypes.c_void_p()
        n = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_rows_drop_sets(
            self.ctx._h, self._h, num_sets, _ptr(flags, c_u8p), ctypes.byref(h), ctypes.byref(n)))
        return Rows(self.ctx, h, n.value, self.ngenomes)

    def prune(self, num_sets, picks, depth=1, fixed=None):
        """catchhip_rows_prune -> (kept, removed): the picks (set ids in pick
        order) examined from the last to the first, one removed whenever every
        base of its rows is covered by more than `depth` of the remaining picks
        and the rows of `fixed` (Rows over the same universes, or None).  kept
        is in pick order, removed in examination order.  The rounds the device
        took are left in `last_prune_rounds`."""
        pk = np.ascontiguousarray(picks, dtype=np.int64)
        flags = np.zeros(max(int(pk.size), 1), dtype=np.uint8)
        nrem = ctypes.c_int64(0)
        rounds = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_rows_prune(
            self.ctx._h, self._h, None if fixed is None else fixed._h, int(num_sets),
            _ptr(pk, c_i64p) if pk.size else None, int(pk.size), int(depth),
            _ptr(flags, c_u8p), ctypes.byref(nrem), ctypes.byref(rounds)))
        gone = flags[:pk.size] != 0
        assert int(gone.sum()) == nrem.value
        self.last_prune_rounds = int(rounds.value)
        return pk[~gone].tolist(), pk[gone][::-1].tolist()

    # checkpoints x universes of one catchhip_rows_pick_gains call stay below this (the library refuses 2^31 and more)
    PICK_GAINS_TABLE_LIMIT = 1 << 31

    def pick_gains(self, num_sets, picks, checkpoints=None, denom=None, covered0=None):
        """catchhip_rows_pick_gains -> (gains uint32[npicks], covered_total
        uint64[ncheck], worst_universe int32[ncheck], worst_covered
        int64[ncheck]); the last three are None without checkpoints.  gains[i] =
        the bases that picks[i] (set ids in pick order) covered first.
        checkpoints: pick counts in [1, npicks], strictly ascending; per
        checkpoint k the bases the first k picks cover (plus covered0[u], per
        universe; None: zeros), in total and in the universe with the smallest
        share of denom[u] (-1: no universe has a positive denom).  A checkpoint
        list whose table would not fit one call is split over several calls;
        the device time and the launches of all of them are left in
        `last_gains_ms` / `last_gains_launches`."""
        pk = np.ascontiguousarray(picks, dtype=np.int64)
        npk = int(pk.size)
        gains = np.zeros(max(npk, 1), dtype=np.uint32)
        self.last_gains_ms, self.last_gains_launches = 0.0, 0

        def fn(*args):
            rc = self.ctx._L.catchhip_rows_pick_gains(*args)
            if rc == 0 and npk:                  # (no picks: the library returns at once, nothing is timed)
                ms, nl = self.ctx.kernel_ms(PHASE_ROWS)
                self.last_gains_ms += ms
                self.last_gains_launches += nl
            return rc
        if checkpoints is None or len(checkpoints) == 0:
            check(fn(self.ctx._h, self._h, int(num_sets), _ptr(pk, c_i64p) if npk else None, npk,
                     _ptr(gains, c_u32p), None, 0, None, None, None, None, None))
            return gains[:npk], None, None, None
        if self.ngenomes is None:
            raise ValueError("pick_gains: rows of an unknown number of universes")
        if denom is None:
            raise ValueError("pick_gains: checkpoints need denom")
        ng = int(self.ngenomes)
        ck = np.ascontiguousarray(checkpoints, dtype=np.int64)
        dn = np.ascontiguousarray(denom, dtype=np.int64)
        c0 = None if covered0 is None else np.ascontiguousarray(covered0, dtype=np.int64)
        if dn.size != ng or (c0 is not None and c0.size != ng):
            raise ValueError("pick_gains: denom / covered0 must hold one value per universe (%d)" % ng)
        if ng == 0:
            dn = np.zeros(1, np.int64)
            c0 = None
        nc = int(ck.size)
        tot = np.zeros(nc, dtype=np.uint64)
        wu = np.zeros(nc, dtype=np.int32)
        wc = np.zeros(nc, dtype=np.int64)
        per_call = max(1, (self.PICK_GAINS_TABLE_LIMIT - 1) // max(ng, 1))
        for lo in range(0, nc, per_call):
            hi = min(nc, lo + per_call)
            part = np.ascontiguousarray(ck[lo:hi])
            t = np.zeros(hi - lo, dtype=np.uint64)
            u = np.zeros(hi - lo, dtype=np.int32)
            c = np.zeros(hi - lo, dtype=np.int64)
            check(fn(self.ctx._h, self._h, int(num_sets), _ptr(pk, c_i64p) if npk else None, npk,
                     _ptr(gains, c_u32p), _ptr(part, c_i64p), hi - lo, _ptr(dn, c_i64p),
                     None if c0 is None else _ptr(c0, c_i64p), _ptr(t, c_u64p), _ptr(u, c_i32p), _ptr(c, c_i64p)))
            tot[lo:hi], wu[lo:hi], wc[lo:hi] = t, u, c
        return gains[:npk], tot, wu, wc

    def fetch_gain0(self, num_sets):
        """catchhip_rows_fetch_gain0 -> uint32[min(num_sets, held)] (None: the rows hold no gain0)."""
        out = np.zeros(max(int(num_sets), 1), dtype=np.uint32)
        held = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_rows_fetch_gain0(self.ctx._h, self._h, int(num_sets), _ptr(out, c_u32p),
                                                    ctypes.byref(held)))
        if held.value == 0:
            return None
        return out[:min(int(num_sets), held.value)]

    def fetch(self):
        n = max(self.n, 1)
        si = np.zeros(n, np.int32); un = np.zeros(n, np.int32)
        st = np.zeros(n, np.int64); en = np.zeros(n, np.int64)
        check(self.ctx._L.catchhip_rows_fetch(
            self.ctx._h, self._h, _ptr(si, c_i32p), _ptr(un, c_i32p),
            _ptr(st, c_i64p), _ptr(en, c_i64p)))
        return si[:self.n], un[:self.n], st[:self.n], en[:self.n]

    def greedy(self, num_sets, ranks=None, universe_p=None):
        """catchhip_setcover_greedy -> picked set ids in pick order."""
        num_sets = int(num_sets)
        out = np.zeros(max(num_sets, 1), dtype=np.int64)
        n_out = ctypes.c_int64(0)
        rk = None if ranks is None else np.ascontiguousarray(ranks, np.int64)
        up = (None if universe_p is None
              else np.ascontiguousarray(universe_p, np.float64))
        check(self.ctx._L.catchhip_setcover_greedy(
            self.ctx._h, self._h, num_sets,
            None if rk is None else _ptr(rk, c_i64p),
            None if up is None else _ptr(up, c_f64p),
            _ptr(out, c_i64p), ctypes.byref(n_out)))
        return out[:n_out.value].tolist()

    def close(self):
        if self._h and self.ctx._h:      # (see Context.close)
            self.ctx._L.catchhip_rows_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BaseMask:
    """The wanted bases of a coordinate space on the device (catchhip_basemask,
    csrc/mask.hip): universes of genome_len[u] bases, and the wanted intervals
    (universe[i], [start[i], end[i]) local to it) in normal form -- sorted by
    (universe, start), non-empty, inside their universe, neither overlapping
    nor touching (anything else: ValueError).  `wanted` (int64 per universe) =
    the wanted bases, counted on the device.  For Rows.restrict and
    Rows.uncovered(mask=...)."""

    def __init__(self, ctx, genome_len, universe, start, end):
        gl = np.ascontiguousarray(genome_len, dtype=np.int64)
        un = np.ascontiguousarray(universe, dtype=np.int32)
        st = np.ascontiguousarray(start, dtype=np.int64)
        en = np.ascontiguousarray(end, dtype=np.int64)
        if not (un.size == st.size == en.size):
            raise ValueError("BaseMask: universe, start and end must have one entry per interval")
        self.ctx = ctx
        self.ngenomes = int(gl.size)
        self.total = int(gl.sum()) if gl.size else 0
        self.n = int(un.size)
        wanted = np.zeros(max(self.ngenomes, 1), dtype=np.int64)
        self._h = ctypes.c_void_p()
        h = ctypes.c_void_p()
        check(ctx._L.catchhip_basemask_create(
            ctx._h, _ptr(gl, c_i64p) if gl.size else None, self.ngenomes,
            _ptr(un, c_i32p) if self.n else None, _ptr(st, c_i64p) if self.n else None,
            _ptr(en, c_i64p) if self.n else None, self.n, ctypes.byref(h), _ptr(wanted, c_i64p)))
        self._h = h
        self.wanted = wanted[:self.ngenomes]
        self.last_build_ms = ctx.kernel_ms(PHASE_ROWS)[0]

    def fetch(self):
        """uint64[(total + 63) // 64]: bit b % 64 of word b // 64 is set iff base
        b is NOT wanted; the bits behind the last base are set."""
        nw = (self.total + 63) // 64
        out = np.zeros(max(nw, 1), dtype=np.uint64)
        check(self.ctx._L.catchhip_basemask_fetch(self.ctx._h, self._h, _ptr(out, c_u64p)))
        return out[:nw]

    def close(self):
        if self._h and self.ctx._h:      # (see Context.close)
            self.ctx._L.catchhip_basemask_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


REDUNDANT_SHIFT, REDUNDANT_LCF = 0, 1
REDUNDANT_MAX_LENGTH = 256    # bases per probe the pair kernel is compiled for (csrc/redundant.hip)


class RedundancyGraph:
    """Device-resident redundancy graph of a probe list (catchhip_redgraph):
    probes i and j are neighbours iff the predicate of `kind` with parameters
    (p0, p1) holds for them -- REDUNDANT_SHIFT: (shift, mismatch_thres);
    REDUNDANT_LCF: (mismatches, lcf_thres >= 1)."""

    def __init__(self, ctx, probe_strs, kind, p0, p1):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        self.n = len(probe_strs)
        buf, off = _concat(list(probe_strs))
        ne = ctypes.c_int64(0)
        check(ctx._L.catchhip_redundancy_graph(
            ctx._h, _ptr(buf, c_u8p), _ptr(off, c_i64p), self.n, int(kind), int(p0), int(p1),
            ctypes.byref(self._h), ctypes.byref(ne)))
        self.nedges = ne.value

    @classmethod
    def _of_pairs(cls, symbol, ctx, strs, above):
        """The graph entry `symbol` of either pair rule."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        buf, off = _concat_records(strs)
        self.n = off.size - 1
        ne = ctypes.c_int64(0)
        check(getattr(ctx._L, symbol)(
            ctx._h, _ptr(buf, c_u8p), _ptr(off, c_i64p), self.n, int(above), ctypes.byref(self._h), ctypes.byref(ne)))
        self.nedges = ne.value
        return self

    @classmethod
    def cross_dimer(cls, ctx, strs, above):
        """catchhip_cross_dimer_graph: records i and j (i != j) are neighbours
        iff run(s_i, s_j) > above (catch_amd/filter/cross_dimer.py; any
        characters, at most REDUNDANT_MAX_LENGTH each, above >= 1)."""
        return cls._of_pairs("catchhip_cross_dimer_graph", ctx, strs, above)

    @classmethod
    def cross_duplex(cls, ctx, strs, above):
        """catchhip_cross_duplex_graph: records i and j (i != j) are neighbours
        iff duplex(s_i, s_j) > above (catch_amd/filter/cross_duplex.py; any
        characters, at most REDUNDANT_MAX_LENGTH each, above >= 0 in hundredths
        of a kcal/mol)."""
        return cls._of_pairs("catchhip_cross_duplex_graph", ctx, strs, above)

    def fetch(self):
        """(ptr int64[n + 1], idx uint32[nedges]): the neighbours of i are
        idx[ptr[i]:ptr[i + 1]], ascending."""
        ptr = np.zeros(self.n + 1, dtype=np.int64)
        idx = np.zeros(max(self.nedges, 1), dtype=np.uint32)
        check(self.ctx._L.catchhip_redundancy_fetch(self.ctx._h, self._h, _ptr(ptr, c_i64p), _ptr(idx, c_u32p)))
        return ptr, idx[:self.nedges]

    def naive(self):
        """catchhip_redundancy_naive -> bool[n]: the probes the reference's
        double loop keeps."""
        keep = np.zeros(max(self.n, 1), dtype=np.uint8)
        check(self.ctx._L.catchhip_redundancy_naive(self.ctx._h, self._h, _ptr(keep, c_u8p)))
        return keep[:self.n].astype(bool)

    def rows(self):
        """catchhip_redundancy_rows -> Rows of the sets {i} + N(i) for
        Rows.greedy(num_sets=n)."""
        h = ctypes.c_void_p()
        n = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_redundancy_rows(self.ctx._h, self._h, ctypes.byref(h), ctypes.byref(n)))
        return Rows(self.ctx, h, n.value)

    def close(self):
        if self._h and self.ctx._h:      # (see Context.close)
            self.ctx._L.catchhip_redundancy_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _concat_records(strs):
    """_concat for records of any characters: what latin-1 cannot hold becomes
    '?', which is no base either."""
    strs = list(strs)
    off = np.zeros(len(strs) + 1, dtype=np.int64)
    if strs:
        np.cumsum([len(s) for s in strs], out=off[1:])
    buf = np.frombuffer("".join(strs).encode("latin-1", "replace"), dtype=np.uint8)
    if buf.size == 0:
        buf = np.zeros(1, dtype=np.uint8)
    return np.ascontiguousarray(buf), off


def _pair_values(symbol, ctx, strs):
    """The one-list values entry `symbol` of either pair rule."""
    buf, off = _concat_records(strs)
    n = off.size - 1
    values = np.zeros(max(n, 1), dtype=np.int32)
    partners = np.full(max(n, 1), -1, dtype=np.int32)
    check(getattr(ctx._L, symbol)(
        ctx._h, _ptr(buf, c_u8p), _ptr(off, c_i64p), n, _ptr(values, c_i32p), _ptr(partners, c_i32p)))
    return values[:n], partners[:n]


def _pair_values_against(symbol, ctx, bs, as_):
    """The two-list values entry `symbol` of either pair rule."""
    b_buf, b_off = _concat_records(bs)
    a_buf, a_off = _concat_records(as_)
    nb = b_off.size - 1
    values = np.zeros(max(nb, 1), dtype=np.int32)
    partners = np.full(max(nb, 1), -1, dtype=np.int32)
    check(getattr(ctx._L, symbol)(
        ctx._h, _ptr(b_buf, c_u8p), _ptr(b_off, c_i64p), nb, _ptr(a_buf, c_u8p), _ptr(a_off, c_i64p),
        a_off.size - 1, _ptr(values, c_i32p), _ptr(partners, c_i32p)))
    return values[:nb], partners[:nb]


def _pair_flags_against(symbol, ctx, bs, as_, above):
    """The two-list flags entry `symbol` of either pair rule."""
    b_buf, b_off = _concat_records(bs)
    a_buf, a_off = _concat_records(as_)
    nb = b_off.size - 1
    flags = np.zeros(max(nb, 1), dtype=np.uint8)
    check(getattr(ctx._L, symbol)(
        ctx._h, _ptr(b_buf, c_u8p), _ptr(b_off, c_i64p), nb, _ptr(a_buf, c_u8p), _ptr(a_off, c_i64p),
        a_off.size - 1, int(above), _ptr(flags, c_u8p)))
    return flags[:nb].astype(bool)


def cross_dimer(ctx, strs):
    """catchhip_cross_dimer -> (values int32[n], partners int32[n]): for every
    record the longest antiparallel pairing with another record of the list
    and the smallest index that reaches it, -1 where the value is 0
    (catch_amd/filter/cross_dimer.py has the definition)."""
    return _pair_values("catchhip_cross_dimer", ctx, strs)


def cross_against(ctx, bs, as_):
    """catchhip_cross_against -> (values int32[len(bs)], partners
    int32[len(bs)]): for every record of `bs` the longest antiparallel pairing
    with a record of `as_` (an equal record included) and the smallest index
    into `as_` that reaches it, -1 where the value is 0
    (catch_amd/filter/cross_dimer.py has the definition)."""
    return _pair_values_against("catchhip_cross_against", ctx, bs, as_)


def cross_against_flags(ctx, bs, as_, above):
    """catchhip_cross_against_flags -> bool[len(bs)]: whether the record of
    `bs` pairs with some record of `as_` over more than `above` (>= 1)
    consecutive bases."""
    return _pair_flags_against("catchhip_cross_against_flags", ctx, bs, as_, above)


def cross_duplex(ctx, strs):
    """catchhip_cross_duplex -> (values int32[n], partners int32[n]): for every
    record the stability of its firmest stretch with another record of the
    list, in hundredths of a kcal/mol, and the smallest index that reaches it,
    -1 where the value is 0 (catch_amd/filter/cross_duplex.py has the
    definition)."""
    return _pair_values("catchhip_cross_duplex", ctx, strs)


def cross_duplex_against(ctx, bs, as_):
    """catchhip_cross_duplex_against -> (values int32[len(bs)], partners
    int32[len(bs)]): cross_against with the stability of the firmest stretch in
    place of the length of the longest."""
    return _pair_values_against("catchhip_cross_duplex_against", ctx, bs, as_)


def cross_duplex_against_flags(ctx, bs, as_, above):
    """catchhip_cross_duplex_against_flags -> bool[len(bs)]: whether the record
    of `bs` forms a stretch firmer than `above` (>= 0, hundredths of a
    kcal/mol) with some record of `as_`."""
    return _pair_flags_against("catchhip_cross_duplex_against_flags", ctx, bs, as_, above)


class Shard:
    """One rank's part of a universe-sharded set cover instance
    (catchhip_shard): the frontier solver's state over this rank's cover
    rows.  Driven round by round by catch_amd.parallel.sharded_solve."""

    def __init__(self, rows, num_sets, ranks=None, universe_p=None, instance_partial=None):
        """universe_p: the fraction to cover of every universe of THIS shard
        (its own genomes, in order), or None = all of each.  With some below 1
        the rounds have a third step (verdict + a second exchange of the lost
        marks; catchhip_shard_create_pi).  instance_partial: whether any
        universe of the WHOLE instance, on whatever rank, is partial -- the
        same value on every rank, so that all of them build the same kind of
        shard (None: decided from this shard's universe_p alone)."""
        self.ctx = rows.ctx
        self.rows = rows                     # keeps the rows alive
        self.num_sets = int(num_sets)
        rk = None if ranks is None else np.ascontiguousarray(ranks, np.int64)
        up = None
        if universe_p is not None:
            # (one entry per universe of the shard's rows: the library reads exactly that many)
            up = np.ascontiguousarray(universe_p, dtype=np.float64)
            if up.size == 0:
                up = None
        self.partial = bool(up is not None and (up < 1.0).any())
        if instance_partial is not None:
            self.partial = bool(instance_partial)
        # whether ANY shard of the instance is partial decides the shape of a round (parallel.sharded_solve) and the
        # kernels of every shard
        self.partial_instance = self.partial
        self._h = ctypes.c_void_p()
        check(self.ctx._L.catchhip_shard_create_pi(
            self.ctx._h, rows._h, self.num_sets,
            None if rk is None else _ptr(rk, c_i64p),
            None if up is None else up.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            -1 if instance_partial is None else int(bool(instance_partial)), ctypes.byref(self._h)))

    def count(self):
        check(self.ctx._L.catchhip_shard_count(self._h))

    def claim_check(self):
        check(self.ctx._L.catchhip_shard_claim_check(self._h))

    def verdict(self):
        """Partial coverage: the local universe tests of this round's candidates
        (failures join the lost marks, which are exchanged once more)."""
        check(self.ctx._L.catchhip_shard_verdict(self._h))

    def apply(self):
        """-> 1 finished, -1 ranks exhausted, 0 another round."""
        done = ctypes.c_int32(0)
        check(self.ctx._L.catchhip_shard_apply(self._h, ctypes.byref(done)))
        return done.value

    def allreduce(self, which):
        """RCCL exchange on the context's communicator (0 gain, 1 lost)."""
        check(self.ctx._L.catchhip_shard_allreduce(self._h, int(which)))

    def _exchange_shape(self):
        """(gain elements, lost elements, lost dtype) of the NEXT exchange: the
        buffers are packed (only the sets alive at the last apply travel), so
        the sizes change from round to round."""
        info = np.zeros(4, dtype=np.int64)
        check(self.ctx._L.catchhip_shard_info(self._h, _ptr(info, c_i64p)))
        return int(info[0]), int(info[1]), (np.uint32 if info[2] == 4 else np.uint8)

    def buffer_to_host(self, which):
        """The gain (uint32) or lost (uint8) exchange buffer."""
        ng, nl, ldt = self._exchange_shape()
        out = np.zeros(ng, dtype=np.uint32) if which == 0 else np.zeros(nl, dtype=ldt)
        if out.size:
            check(self.ctx._L.catchhip_shard_buffer_copy(
                self._h, int(which), out.ctypes.data_as(ctypes.c_void_p), 1))
        return out

    def buffer_from_host(self, which, arr):
        ng, nl, ldt = self._exchange_shape()
        a = np.ascontiguousarray(arr, dtype=np.uint32 if which == 0 else ldt)
        assert a.size == (ng if which == 0 else nl)
        if a.size:
            check(self.ctx._L.catchhip_shard_buffer_copy(
                self._h, int(which), a.ctypes.data_as(ctypes.c_void_p), 0))

    def picks(self):
        out = np.zeros(max(self.num_sets, 1), dtype=np.int64)
        n = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_shard_picks(self._h, _ptr(out, c_i64p),
                                               ctypes.byref(n)))
        return out[:n.value].tolist()

    def close(self):
        if self._h and self.ctx._h:      # (see Context.close)
            self.ctx._L.catchhip_shard_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shards_solve(shards, transport, rounds_per_sync=4):
    """catchhip_shard_solve: the whole round loop of the instance under the C ABI, `rounds_per_sync` rounds per host
    read-back.  transport "rccl": one shard, exchanges over its context's communicator; "local": the shards of this
    process (one context) exchange among themselves.  Returns the picks in the sequential pick order."""
    arr = (ctypes.c_void_p * len(shards))(*[s._h for s in shards])
    done = ctypes.c_int32(0)
    check(shards[0].ctx._L.catchhip_shard_solve(len(shards), arr, 0 if transport == "rccl" else 1, int(rounds_per_sync),
                                                 ctypes.byref(done)))
    out = [sh.picks() for sh in shards]
    if any(o != out[0] for o in out):
        raise RuntimeError("sharded solve: shards returned different picks")
    return out[0]


def shards_allreduce_local(shards, which):
    """catchhip_shard_allreduce_local: the exchange between shards that live
    in this process on one device."""
    arr = (ctypes.c_void_p * len(shards))(*[s._h for s in shards])
    check(shards[0].ctx._L.catchhip_shard_allreduce_local(len(shards), arr,
                                                         int(which)))


class Signatures:
    """Device-resident MinHash signatures of sequences (catchhip_sigs): the N
    smallest values of (a * md5(kmer) + b) mod (2^31 - 1) per sequence."""

    def __init__(self, ctx, seqs, kmer_size, N, a, b):
        self.ctx = ctx
        self.n = len(seqs)
        self.N = int(N)
        self._h = ctypes.c_void_p()
        ptrs = _str_pointers(seqs) if self.n else None
        if ptrs is not None:
            # one pointer per sequence: gathered by the library's host threads (no join + encode of gigabytes here)
            arr, lens = ptrs
            check(ctx._L.catchhip_sigs_create_ptrs(
                ctx._h, ctypes.cast(arr, ctypes.c_void_p), _ptr(lens, c_i64p), self.n, int(kmer_size), self.N,
                int(a), int(b), ctypes.byref(self._h)))
            return
        try:
            raw = "".join(seqs).encode("ascii")
        except UnicodeEncodeError:
            raise ValueError("sequences must be ASCII")
        buf = np.frombuffer(raw, dtype=np.uint8)
        if buf.size == 0:
            buf = np.zeros(1, dtype=np.uint8)
        off = np.zeros(self.n + 1, dtype=np.uint64)
        if seqs:
            np.cumsum([len(s) for s in seqs], out=off[1:])
        self._h = ctypes.c_void_p()
        check(ctx._L.catchhip_sigs_create(
            ctx._h, _ptr(np.ascontiguousarray(buf), c_u8p), _ptr(off, c_u64p),
            self.n, int(kmer_size), self.N, int(a), int(b),
            ctypes.byref(self._h)))

    def close(self):
        if self._h and self.ctx._h:      # (see Context.close)
            self.ctx._L.catchhip_sigs_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def fetch(self):
        """(n, N) uint32, each row ascending."""
        out = np.zeros((max(self.n, 1), self.N), dtype=np.uint32)
        check(self.ctx._L.catchhip_sigs_fetch(self.ctx._h, self._h,
                                              _ptr(out, c_u32p)))
        return out[:self.n]

    def common_row(self, j):
        """values signature j shares with every signature under the N-step
        merge walk of estimate_jaccard_dist (uint16[n])."""
        out = np.zeros(max(self.n, 1), dtype=np.uint16)
        check(self.ctx._L.catchhip_sigs_common_row(self.ctx._h, self._h,
                                                   int(j), _ptr(out, c_u16p)))
        return out[:self.n]

    def neighbors(self, j, min_common):
        """catchhip_sigs_neighbors -> (indices ascending, their common counts):
        the sequences whose merge walk against signature j finds at least
        min_common shared values."""
        if not hasattr(self, "_nb_buf"):
            self._nb_buf = np.zeros(max(self.n, 1), dtype=np.uint64)
        cnt = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_sigs_neighbors(
            self.ctx._h, self._h, int(j), int(min_common), _ptr(self._nb_buf, c_u64p),
            int(self._nb_buf.size), ctypes.byref(cnt)))
        got = np.sort(self._nb_buf[:cnt.value])
        return (got >> np.uint64(16)).astype(np.int64), (got & np.uint64(0xffff)).astype(np.int64)

    NEIGHBORS_MANY_MAX = 32        # queries per call (NEIGH_MAXQ), signatures of at most 112 values

    def neighbors_many(self, js, min_common):
        """catchhip_sigs_neighbors_many -> list of (indices ascending, their
        common counts), one per vertex of js (at most NEIGHBORS_MANY_MAX)."""
        js = np.ascontiguousarray(js, dtype=np.uint32)
        if not hasattr(self, "_nbm_buf"):
            self._nbm_buf = np.zeros(max(4 * self.n, 1 << 16), dtype=np.uint64)
        cnt = ctypes.c_int64(0)
        while True:
            rc = self.ctx._L.catchhip_sigs_neighbors_many(
                self.ctx._h, self._h, _ptr(js, c_u32p), int(js.size), int(min_common),
                _ptr(self._nbm_buf, c_u64p), int(self._nbm_buf.size), ctypes.byref(cnt))
            if rc != 0 and cnt.value > self._nbm_buf.size:      # more neighbours than room: grow and ask again
                self._nbm_buf = np.zeros(int(cnt.value) + (1 << 16), dtype=np.uint64)
                continue
            check(rc)
            break
        got = np.sort(self._nbm_buf[:cnt.value])                # by query, then by index
        q = (got >> np.uint64(48)).astype(np.int64)
        bounds = np.searchsorted(q, np.arange(js.size + 1))
        idx = ((got >> np.uint64(16)) & np.uint64(0xffffffff)).astype(np.int64)
        com = (got & np.uint64(0xffff)).astype(np.int64)
        return [(idx[bounds[i]:bounds[i + 1]], com[bounds[i]:bounds[i + 1]]) for i in range(js.size)]

    GRAPH_MAX_EDGES = 1 << 29      # ordered pairs kept as a graph (6 GB on the device while sorting, 4 GB on the host)

    def graph(self, min_common):
        """catchhip_sigs_graph + fetch -> (ptr int64[n + 1], idx uint32[E] ascending inside a row, common
        uint32[E]): the neighbour lists of every vertex in one device pass, or None when there are more than
        GRAPH_MAX_EDGES ordered pairs (the caller then asks list by list).  Signatures of at most 112 values."""
        cnt = ctypes.c_int64(0)
        check(self.ctx._L.catchhip_sigs_graph(self.ctx._h, self._h, int(min_common), int(self.GRAPH_MAX_EDGES),
                                              ctypes.byref(cnt)))
        e = int(cnt.value)
        if e > self.GRAPH_MAX_EDGES:
            return None
        ptr = np.zeros(self.n + 1, dtype=np.int64)
        idx = np.empty(max(e, 1), dtype=np.uint32)
        com = np.empty(max(e, 1), dtype=np.uint32)
        check(self.ctx._L.catchhip_sigs_graph_fetch(self.ctx._h, self._h, _ptr(ptr, c_i64p), _ptr(idx, c_u32p),
                                                    _ptr(com, c_u32p)))
        return ptr, idx[:e], com[:e]

    def condensed(self, lut):
        """float32[n(n-1)/2] in SciPy's condensed order; entry = lut[common]."""
        lut = np.ascontiguousarray(lut, dtype=np.float32)
        assert lut.size == self.N + 1
        npairs = self.n * (self.n - 1) // 2
        out = np.zeros(max(npairs, 1), dtype=np.float32)
        check(self.ctx._L.catchhip_sigs_condensed(
            self.ctx._h, self._h, _ptr(lut, c_f32p), _ptr(out, c_f32p)))
        return out[:npairs]

    def linkage_fits(self):
        """Whether the float64 square matrix of linkage_clusters (8 n^2 bytes) takes at most half of the device
        memory that is free now."""
        fits = ctypes.c_int32(0)
        check(self.ctx._L.catchhip_linkage_fits(self.ctx._h, self.n, ctypes.byref(fits)))
        return bool(fits.value)

    def linkage_clusters(self, lut, threshold, return_merges=False):
        """catchhip_sigs_linkage_average: SciPy's average linkage + fcluster(criterion="distance") of the
        distances lut[common] on the device -> clusters as lists of indices, largest first (what
        cluster.cluster_hierarchically_from_dist_matrix returns for self.condensed(lut)); return_merges: also the
        linkage matrix, float64 (n - 1, 4)."""
        from catch_amd.utils import cluster
        lut = np.ascontiguousarray(lut, dtype=np.float32)
        assert lut.size == self.N + 1
        labels = np.zeros(max(self.n, 1), dtype=np.int32)
        merges = np.zeros((max(self.n - 1, 1), 4), dtype=np.float64) if return_merges else None
        check(self.ctx._L.catchhip_sigs_linkage_average(
            self.ctx._h, self._h, _ptr(lut, c_f32p), float(threshold), _ptr(labels, c_i32p),
            _ptr(merges, c_f64p) if return_merges else None))
        clusters = cluster._clusters_from_labels(labels[:self.n])
        return (clusters, merges[:max(self.n - 1, 0)]) if return_merges else clusters


def tolerant_bp(ctx, probes, targets, mismatches, lcf_thres, island, out):
    """catchhip_tolerant_bp: out (int64, one per unique probe) += bp."""
    check(ctx._L.catchhip_tolerant_bp(ctx._h, probes._h, targets._h,
                                      int(mismatches), int(lcf_thres),
                                      int(island), _ptr(out, c_i64p)))


def setcover_filter(ctx, probes, targets, mismatches, lcf_thres, island,
                    cover_extension, num_sets, ranks=None, universe_p=None,
                    mode=SCAN_AUTO, as_array=False):
    """catchhip_setcover_filter: scan + greedy in one call.
    Returns (picked set ids in pick order, number of cover rows); as_array: the
    ids as an int64 array instead of a list (a union instance makes 10^5 picks:
    list conversions there and back were 8 ms of a 100-ms step)."""
    return setcover_filter_many([(ctx, probes, targets, num_sets, ranks,
                                  universe_p)], mismatches, lcf_thres, island,
                                cover_extension, mode, as_array)[0]


def setcover_filter_many(groups, mismatches, lcf_thres, island,
                         cover_extension, mode=SCAN_AUTO, as_array=False):
    """catchhip_setcover_filter_many over independent groups, each a tuple
    (ctx, probes, targets, num_sets, ranks or None, universe_p or None) with
    its own Context.  Returns [(ids, nrows)] per group."""
    n = len(groups)
    if n == 0:
        return []
    L = groups[0][0]._L
    VP = ctypes.c_void_p
    ctxs = (VP * n)(*[g[0]._h for g in groups])
    prs = (VP * n)(*[g[1]._h for g in groups])
    tgs = (VP * n)(*[g[2]._h for g in groups])
    nsets = np.array([int(g[3]) for g in groups], dtype=np.int64)
    outs = [np.zeros(max(int(g[3]), 1), dtype=np.int64) for g in groups]
    rks = [None if g[4] is None else np.ascontiguousarray(g[4], np.int64)
           for g in groups]
    ups = [None if g[5] is None else np.ascontiguousarray(g[5], np.float64)
           for g in groups]
    out_p = (c_i64p * n)(*[_ptr(o, c_i64p) for o in outs])
    rk_p = (c_i64p * n)(*[None if r is None else _ptr(r, c_i64p) for r in rks])
    up_p = (c_f64p * n)(*[None if u is None else _ptr(u, c_f64p) for u in ups])
    n_out = np.zeros(n, dtype=np.int64)
    nrows = np.zeros(n, dtype=np.int64)
    if n == 1:
        check(L.catchhip_setcover_filter(
            ctxs[0], prs[0], tgs[0], int(mismatches), int(lcf_thres),
            int(island), int(cover_extension), int(mode), int(nsets[0]),
            rk_p[0], up_p[0], out_p[0], _ptr(n_out, c_i64p),
            _ptr(nrows, c_i64p)))
    else:
        check(L.catchhip_setcover_filter_many(
            n, ctxs, prs, tgs, int(mismatches), int(lcf_thres), int(island),
            int(cover_extension), int(mode), _ptr(nsets, c_i64p), rk_p, up_p,
            out_p, _ptr(n_out, c_i64p), _ptr(nrows, c_i64p)))
    res = [((outs[g][:n_out[g]].copy() if as_array else outs[g][:n_out[g]].tolist()), int(nrows[g])) for g in range(n)]
    if _solution_checks is not None:
        # bench / tests: every instance's picks replayed by the independent check kernels (one more scan, untimed)
        for g, (ids, _) in zip(groups, res):
            rows = Rows.scan(g[0], g[1], g[2], mismatches, lcf_thres, island, cover_extension, mode)
            try:
                r = rows.cover_check(g[3], ids, g[5])
                r.update(picks=len(ids), rows=rows.n, universes=int(g[2].ngenomes))
                _solution_checks.append(r)
            finally:
                rows.close()
    return res


_solution_checks = None


def setcover_grid(ctx, probes, targets, mismatches, lcf_thres, island,
                  cover_extensions, num_sets, ranks=None, universe_p=None,
                  mode=SCAN_AUTO):
    """catchhip_setcover_grid: one scan at cover extension 0, the rows at
    every extension derived from it and solved.  Returns [(picked set ids in
    pick order, number of cover rows)] per extension."""
    ext = np.ascontiguousarray(cover_extensions, dtype=np.int32)
    n = int(ext.size)
    num_sets = int(num_sets)
    outs = [np.zeros(max(num_sets, 1), dtype=np.int64) for _ in range(n)]
    out_p = (c_i64p * max(n, 1))(*[_ptr(o, c_i64p) for o in outs])
    n_out = np.zeros(max(n, 1), dtype=np.int64)
    nrows = np.zeros(max(n, 1), dtype=np.int64)
    rk = None if ranks is None else np.ascontiguousarray(ranks, np.int64)
    up = None if universe_p is None else np.ascontiguousarray(universe_p, np.float64)
    check(ctx._L.catchhip_setcover_grid(
        ctx._h, probes._h, targets._h, int(mismatches), int(lcf_thres),
        int(island), int(mode), n, _ptr(ext, c_i32p) if n else None, num_sets,
        None if rk is None else _ptr(rk, c_i64p),
        None if up is None else _ptr(up, c_f64p), out_p,
        _ptr(n_out, c_i64p), _ptr(nrows, c_i64p)))
    return [(outs[i][:n_out[i]].tolist(), int(nrows[i])) for i in range(n)]


def pool_solve(ctx, opt_off, counts, losses, budget):
    """catchhip_pool_solve: the exact budgeted choice of one option per dataset.
    opt_off[D + 1], counts / losses per option -> (option index per dataset,
    total count, loss).  ValueError when the budget cannot be met."""
    off = np.ascontiguousarray(opt_off, dtype=np.int64)
    cn = np.ascontiguousarray(counts, dtype=np.int64)
    ls = np.ascontiguousarray(losses, dtype=np.float64)
    D = int(off.size) - 1
    assert D >= 0 and cn.size == ls.size == int(off[-1])
    if cn.size == 0:
        cn, ls = np.zeros(1, np.int64), np.zeros(1, np.float64)
    out = np.zeros(max(D, 1), dtype=np.int32)
    total = ctypes.c_int64(0)
    loss = ctypes.c_double(0.0)
    check(ctx._L.catchhip_pool_solve(ctx._h, D, _ptr(off, c_i64p), _ptr(cn, c_i64p), _ptr(ls, c_f64p),
                                     int(budget), _ptr(out, c_i32p), ctypes.byref(total), ctypes.byref(loss)))
    return out[:D].astype(np.int64), int(total.value), float(loss.value)


def collect_solution_checks(sink):
    """sink: a list -- from now on every fused scan + solve (setcover_filter / _many) is followed by
    catchhip_rows_cover_check on a second scan of the same instance and its verdict is appended; None: off."""
    global _solution_checks
    _solution_checks = sink


class Prefetch:
    """Runs build(item) for the items in order on a helper thread, at most
    `depth` finished results ahead of the consumer: the packing and upload of
    group i + 1 (host gather into pinned memory, H2D, the front-end kernels on
    the upload context's stream) overlap the scan and solve of group i on the
    compute context.  Iterating yields (item, result) in order; an exception in
    build() is re-raised at the consumer.  close() stops the helper and hands
    every result that was built but not consumed to `discard`."""

    def __init__(self, items, build, depth=2, discard=None):
        import queue
        import threading
        self._q = queue.Queue(maxsize=max(1, int(depth)))
        self._stop = threading.Event()
        self._discard = discard
        self._items = list(items)

        def run():
            for it in self._items:
                if self._stop.is_set():
                    break
                try:
                    res, err = build(it), None
                except BaseException as e:      # handed to the consumer
                    res, err = None, e
                taken = False
                while not self._stop.is_set():
                    try:
                        self._q.put((it, res, err), timeout=0.05)
                        taken = True
                        break
                    except queue.Full:
                        continue
                if not taken and res is not None and self._discard:
                    self._discard(res)          # stopped before it was handed over
                if err is not None:
                    break

        self._thread = threading.Thread(target=run, name="catchhip-prefetch",
                                        daemon=True)
        self._thread.start()

    def __iter__(self):
        for _ in range(len(self._items)):
            it, res, err = self._q.get()
            if err is not None:
                raise err
            yield it, res

    def close(self):
        import queue
        self._stop.set()
        self._thread.join()
        while True:
            try:
                _it, res, _err = self._q.get_nowait()
            except queue.Empty:
                break
            if res is not None and self._discard:
                self._discard(res)


class PrefetchPool:
    """Prefetch with several helper threads: build(item, worker) runs on `workers`
    threads, items are taken in order and results are handed to the consumer in
    order; at most workers + depth items are built or waiting at any time.  For
    stages whose calls leave the device idle much of the time (the MinHash
    filter's ~45 dependent rounds): two of them on two streams overlap."""

    def __init__(self, items, build, workers=2, depth=1, discard=None):
        import threading
        self._items = list(items)
        n = len(self._items)
        self._res = [None] * n
        self._ready = [threading.Event() for _ in range(n)]
        self._stop = threading.Event()
        self._discard = discard
        self._lock = threading.Lock()
        self._next = 0
        self._taken = 0                       # results the consumer has taken
        self._room = threading.Semaphore(max(1, int(workers)) + max(0, int(depth)))

        def run(w):
            while not self._stop.is_set():
                if not self._room.acquire(timeout=0.05):
                    continue
                with self._lock:
                    i = self._next
                    self._next += 1
                if i >= n or self._stop.is_set():
                    self._room.release()
                    return
                try:
                    res, err = build(self._items[i], w), None
                except BaseException as e:      # handed to the consumer
                    res, err = None, e
                self._res[i] = (res, err)
                self._ready[i].set()
                if err is not None:
                    self._stop.set()
                    return

        self._threads = [threading.Thread(target=run, args=(w,), name="catchhip-prefetch-%d" % w, daemon=True)
                         for w in range(max(1, int(workers)))]
        for t in self._threads:
            t.start()

    def __iter__(self):
        for i in range(len(self._items)):
            while not self._ready[i].wait(0.05):
                if self._stop.is_set() and not self._ready[i].is_set():
                    # a later item failed before this one was built: report that failure
                    for r in self._res:
                        if r is not None and r[1] is not None:
                            raise r[1]
            res, err = self._res[i]
            self._res[i] = None
            self._taken = i + 1
            self._room.release()
            if err is not None:
                raise err
            yield self._items[i], res

    def close(self):
        self._stop.set()
        for t in self._threads:
            t.join()
        for i in range(self._taken, len(self._items)):
            r, self._res[i] = self._res[i], None
            if r is not None and r[0] is not None and self._discard:
                self._discard(r[0])


_upload_ctxs = {}


def upload_context(device=None, index=0):
    """The context whose stream packs and uploads the NEXT group's inputs while
    the compute context works (made on first use; index: further ones for
    stages that run several builders side by side)."""
    if device is None:
        device = default_context().device
    if (device, index) not in _upload_ctxs:
        _upload_ctxs[(device, index)] = Context(device)
    return _upload_ctxs[(device, index)]


_default_ctx = None


def default_context():
    """Process-wide context on the device selected by CATCHHIP_DEVICE /
    LOCAL_RANK (one process per GPU)."""
    global _default_ctx
    if _default_ctx is None:
        import os
        dev = int(os.environ.get("CATCHHIP_DEVICE",
                                 os.environ.get("LOCAL_RANK", "0")))
        _default_ctx = Context(dev)
    return _default_ctx
