// cec_pool.inc -- background recovery of many small unit ranges (SURVEY §8f rank 2).
// Included by cec_runtime.hip after cec_recovery.inc; not a separate TU.  Every buffer
// is a Buf (cec_cache.inc); fold_updates takes its waves from colour_intervals
// (cec_hostplan.hpp), its launch windows from WaveTiles (cec_runtime.hip) and its
// failure guard from InFlight (cec_cache.inc).  Which request owns which slots, what is
// queued, ready or solved and what a flush does with whom is poolbook::Book's
// (cec_poolbook.hpp, no device); here are the buffers, combinations, tiles and launches.
//
// The idle recoverer (idle_event_handler, memcached.c:5712-5734) issues one 4 KiB unit
// per request (do_recovery(NULL, s, s)) with up to TOO_MANY_RECOVERY = 85 in flight
// (const.h:27).  Per request the reference folds each data peer's reply
// (complete_recovery_nread -> recovery_recover_units, memcached.c:2596-2651 ->
// recovery.c:61-96) and the leader solves (complete_recovery_bottom_half).  A
// cec_recovery session per unit would pay a synchronous launch per reply; a pool
// instead keeps every in-flight request's residual in one HBM buffer and folds all
// queued replies in ONE launch per flush:
//
//   slots     residual R[capacity][4 KiB] in HBM; a request owns nunits contiguous slots
//   replies   add_peer copies the peer's units into that peer's pinned, device-mapped
//             staging Q_j at the request's slots (a host memcpy, no launch)
//   flush     one combine launch over every request with queued replies:
//               R[slot] = (first touch ? P[off] : R[slot]) ^ sum_{j queued} c_j * Q_j[slot]
//             tiles carry off = the arena offset (P) and src_off = the slot offset (R, Q_j),
//             the kernel reads Q_j over PCIe (zero-copy); one pattern per (peer set, touch)
//   solve     one launch over the listed single-loss requests of this leader:
//               out[lost][off] = inv * R[slot]
//             or, for a server whose recovery state stays on the host (the _host calls),
//               O[slot] = inv * R[slot] into the pool's own mapped pinned output O, which
//             the host reads in place (no arena is written: the caller decides which
//             units to fill, as fill_completed_recovered_data skips sub_flags == 2)
//   n losses  a request that loses n >= 2 data lids is led by this pool once the other
//             n - 1 participating parities' residuals have been given (add_residual: what
//             recover_units_gather receives into data_from_parity[lid], memcached.c:
//             4190-4219, and complete_recovery_bottom_half puts into C[], :7881-7888).  They
//             lie in one more mapped pinned staging G_p per parity lid, at the request's
//             slots, and the solve is the combination cec_recovery_finish builds:
//               out[lost_x] = sum_p inv[x][p] * C[p],  C[self] = R[slot], C[p] = G_p[slot]
//             four shards a launch.  A flush that makes such a request ready (its last
//             reply or its last residual) solves it in its own launch up to three losses
//             (R' and the shards are the launch's four outputs); past three the solve's
//             launches follow the flush's in the same call and read the new R from HBM.
//   no data   with k <= m a mask may name parities only.  No reply comes, so begin queues the
//             request's first touch itself: the next flush writes R[slot] = P[off] (the pattern
//             of no queued reply with the first touch, the parity its only input) and, if it
//             solves and the other residuals are in, the k shards in the same launch (k <= 3)
//             or behind it.  solve, residual and fold_update(s) flush first, so none reads the
//             slots before that; an explicit solve that still has a first touch to make is
//             that one flush launch ahead of its ceil(n / 4).
//   updates   fold_update flushes first, so a queued reply is folded exactly when the
//             reference would have folded it (before the next parity change), then
//             R ^= c * diff where the request is touched and the peer has not contributed
//             (recovery_try_update_unit, recovery.c:99-131; any data lid, in the mask
//             or not).

// The pool's own coefficient tables for its flushes: an append-only device blob
// [patterns (cap_pats)][LDS engine rows (cap_rows bytes)], kept OUT of the LRU cache.
// (Launching every flush with the whole growing table through the cache made one cache
// key per table version: at k = 6 up to 896 versions of up to 1.5 MiB, which forced
// evictions, each a device-wide synchronisation.)  Every pool call ends synchronously
// (stream_wait), so when a call starts nothing of the pool's is in flight: a new
// pattern is written into the pinned mirror and only its bytes are uploaded, on the
// call's stream ahead of its launch; outgrowing the blob re-uploads it whole into a
// buffer twice the size and returns the old (idle) one to the cache.
struct PoolTables {
    int dev = -1, engine = -1;
    std::vector<Pattern> pats;  // host copy, index = tile pattern index
    std::vector<uint8_t> rows;  // LDS engine product rows (pattern lds_row_base indexes these)
    size_t cap_pats = 0, cap_rows = 0;        // device blob capacity
    size_t synced_pats = 0, synced_rows = 0;  // prefix already uploaded
    Buf d, h;                                 // device blob, pinned mirror

    void release() {
        d.release();
        h.release();
        cap_pats = cap_rows = synced_pats = synced_rows = 0;
    }
    void reset(int dev_, int engine_) {  // (idle: see above)
        release();
        pats.clear();
        rows.clear();
        dev = dev_;
        engine = engine_;
    }
    // Device copy current for every pattern appended so far (async on s).
    int sync(hipStream_t s) {
        if (pats.size() > cap_pats || rows.size() > cap_rows) {
            const size_t np = std::max<size_t>({16, 2 * cap_pats, pats.size()});
            const size_t nr = std::max<size_t>({4096, 2 * cap_rows, (rows.size() + 4095) & ~size_t(4095)});
            const size_t nb = np * sizeof(Pattern) + nr;
            Buf nd, nh;
            if (!nd.acquire(dev_cache(), dev, nb) || !nh.acquire(pin_cache(), dev, nb))
                return fail(CEC_ENOMEM, "recovery pool: %zu bytes of coefficient tables", nb);
            release();
            d = std::move(nd);
            h = std::move(nh);
            cap_pats = np;
            cap_rows = nr;
        }
        const size_t rbase = cap_pats * sizeof(Pattern);
        if (synced_pats < pats.size()) {
            const size_t o = synced_pats * sizeof(Pattern), n = (pats.size() - synced_pats) * sizeof(Pattern);
            memcpy(h.get() + o, pats.data() + synced_pats, n);
            HIP_TRY(hipMemcpyAsync(d.get() + o, h.get() + o, n, hipMemcpyHostToDevice, s));
            synced_pats = pats.size();
        }
        if (synced_rows < rows.size()) {
            const size_t o = rbase + synced_rows, n = rows.size() - synced_rows;
            memcpy(h.get() + o, rows.data() + synced_rows, n);
            HIP_TRY(hipMemcpyAsync(d.get() + o, h.get() + o, n, hipMemcpyHostToDevice, s));
            synced_rows = rows.size();
        }
        return CEC_OK;
    }
};

struct cec_recovery_pool {
    int device = -1;
    std::vector<int> matrix;
    Code code;  // over `matrix`
    const uint8_t *parity = nullptr;  // this parity's arena (device)
    Buf residual;      // device, capacity * kTile
    Buf q[CEC_MAX_K];  // per data lid: pinned, mapped, capacity * kTile
    // capacity tiles (one flush / solve), mapped pinned: the kernel reads them in place over
    // PCIe (no upload ahead of each launch), through the buffer's device alias
    Buf tiles;
    Buf diff;  // pinned mapped staging for diffs
    // _host solves: plane x holds the x-th lost lid's rebuilt units at the request's slots;
    // mapped pinned, capacity * kTile each, on first use
    Buf out[CEC_MAX_M];
    // given residuals of the other participating parities (multi-loss requests), by parity
    // index: mapped pinned, capacity * kTile each, on first use of that parity
    Buf given[CEC_MAX_M];
    poolbook::Book book;  // the requests, their slots and the queue; k, m, this parity's lid, the capacity
    // The flush patterns seen so far: poolbook::flush_key -> index into `tables` (the pool's
    // own).  One per (queued peer set, first touch) for the requests a flush only folds, at
    // most 2^k * 2; and for those it also solves one per (queued peer set, first touch, mask,
    // to_host) -- the mask, not the lost lid alone: it names the parities whose residuals
    // come in and decides the inverse -- at most 2^(k-n) * 2 * 2 per mask of n <= 3 losses,
    // C(k,n) * C(m-1,n-1) masks per n (this parity is in every one).
    std::map<uint64_t, int> flush_pat;
    PoolTables tables;
    Tracker uses;  // the streams of its calls (destroy waits for those only)
};

CEC_API int cec_recovery_pool_destroy(cec_recovery_pool *p) {
    if (!p) return CEC_OK;
    (void)p->uses.wait(p->device);  // the pool's own work, not the device
    delete p;                       // (its buffers go back to the caches)
    return CEC_OK;
}

CEC_API int cec_recovery_pool_release_stream(cec_recovery_pool *p, void *stream) {
    if (!p) return fail(CEC_EINVAL, "cec_recovery_pool_release_stream: pool is NULL");
    if (hipError_t e = p->uses.release(p->device, static_cast<hipStream_t>(stream)); e != hipSuccess)
        return fail(CEC_EHIP, "cec_recovery_pool_release_stream: %s", hipGetErrorString(e));
    return CEC_OK;
}

CEC_API int cec_recovery_pool_create(cec_recovery_pool **out, int k, int m, const int *matrix,
                                     int lid_self, const uint8_t *parity_arena, int capacity_units) {
    if (!out) return fail(CEC_EINVAL, "cec_recovery_pool_create: out is NULL");
    *out = nullptr;
    if (int r = check_code(k, m, matrix)) return r;
    if (lid_self < k || lid_self >= k + m || !parity_arena || capacity_units < 1 ||
        capacity_units > (1 << 20))
        return fail(CEC_EINVAL, "cec_recovery_pool_create: bad lid %d / arena / capacity %d", lid_self,
                    capacity_units);
    int dev;
    if (int r = current_device(&dev)) return r;
    cec_recovery_pool *p = new (std::nothrow) cec_recovery_pool;
    if (!p) return fail(CEC_ENOMEM, "cec_recovery_pool_create: host allocation");
    p->device = dev;
    p->code = Code::owned(p->matrix, k, m, matrix);
    p->parity = parity_arena;
    const size_t bytes = static_cast<size_t>(capacity_units) * kTile;
    bool ok = p->residual.acquire(dev_cache(), dev, bytes) && p->tiles.acquire_mapped(dev, capacity_units * sizeof(Tile));
    for (int j = 0; j < k && ok; ++j) ok = p->q[j].acquire_mapped(dev, bytes);
    if (!ok) {
        cec_recovery_pool_destroy(p);
        return fail(CEC_ENOMEM, "cec_recovery_pool_create: %d units of residual and staging", capacity_units);
    }
    p->book = poolbook::Book(k, m, lid_self, capacity_units);
    p->tables.dev = dev;
    *out = p;
    return CEC_OK;
}

static_assert(poolbook::kMaxK == CEC_MAX_K && poolbook::kMaxM == CEC_MAX_M && poolbook::kStreams == kMaxStreams &&
                  poolbook::kInputs == kPatN && poolbook::kOutputs == kPatL && poolbook::kUnit == kTile,
              "cec_poolbook.hpp's limits");

static const poolbook::Req *pool_find(const cec_recovery_pool *p, int id) { return p ? p->book.find(id) : nullptr; }

CEC_API int cec_recovery_pool_begin(cec_recovery_pool *p, uint32_t mask, int unit_begin, int unit_end) {
    const int id = p ? p->book.begin(mask, unit_begin, unit_end) : -poolbook::kBadArgs;
    if (id == -poolbook::kBadArgs)
        return fail(CEC_EINVAL, "cec_recovery_pool_begin: bad mask 0x%x / units [%d, %d]", mask, unit_begin,
                    unit_end);
    const int n = unit_end - unit_begin + 1;
    if (id == -poolbook::kTooLarge) return fail(CEC_EFULL, "cec_recovery_pool_begin: %d units > capacity", n);
    if (id < 0) return fail(CEC_EFULL, "cec_recovery_pool_begin: no %d free contiguous units", n);
    return id;
}

// A checked reply into the peer's staging at the request's slots, then noted.
static int pool_take_reply(cec_recovery_pool *p, int id, int peer, const void *units) {
    const poolbook::Req &r = p->book.reqs[id];
    const size_t off = static_cast<size_t>(r.slot) * kTile, len = static_cast<size_t>(r.nunits) * kTile;
    uint8_t *const q = p->q[peer].get() + off;
    if (units == q) {
        // received in place (cec_recovery_pool_staging): nothing to copy
    } else if (const void *dv = device_view_of(units)) {  // device-resident reply: copy on the device
        int dev;
        if (int rc = current_device(&dev)) return rc;
        HIP_TRY(hipMemcpy(q, dv, len, hipMemcpyDefault));
    } else {
        memcpy(q, units, len);
    }
    p->book.note_reply(id, peer);
    return CEC_OK;
}

CEC_API int cec_recovery_pool_add_peer(cec_recovery_pool *p, int id, int peer, const void *units) {
    const poolbook::Refusal why = p ? p->book.check_reply(id, peer, units) : poolbook::kNoReply;
    if (why == poolbook::kNoReply)
        return fail(CEC_EINVAL, "cec_recovery_pool_add_peer: request %d / peer %d", id, peer);
    if (why) return fail(CEC_EINVAL, "cec_recovery_pool_add_peer: peer %d already applied (recovery.c:75)", peer);
    return pool_take_reply(p, id, peer, units);
}

// An event-loop pass's replies in one call: every (ids[i], peers[i]) checked as add_peer
// checks it -- and no pair twice -- before any is queued, then queued in list order.
CEC_API int cec_recovery_pool_add_peers(cec_recovery_pool *p, const int *ids, const int *peers,
                                        const void *const *units, int n) {
    if (!p || n < 0 || (n > 0 && (!ids || !peers || !units)))
        return fail(CEC_EINVAL, "cec_recovery_pool_add_peers: bad args");
    int i = 0;
    const poolbook::Refusal why = p->book.check_replies(ids, peers, units, n, &i);
    if (why == poolbook::kNoReply)
        return fail(CEC_EINVAL, "cec_recovery_pool_add_peers: reply %d: request %d / peer %d", i, ids[i], peers[i]);
    if (why == poolbook::kApplied)
        return fail(CEC_EINVAL, "cec_recovery_pool_add_peers: reply %d: peer %d already applied (recovery.c:75)", i,
                    peers[i]);
    if (why) return fail(CEC_EINVAL, "cec_recovery_pool_add_peers: a (request, peer) pair listed twice");
    for (i = 0; i < n; ++i)
        if (int rc = pool_take_reply(p, ids[i], peers[i], units[i])) return rc;  // (HIP copy only)
    return CEC_OK;
}

CEC_API uint8_t *cec_recovery_pool_staging(cec_recovery_pool *p, int id, int peer, size_t *len) {
    const poolbook::Req *r = pool_find(p, id);
    if (!r || peer < 0 || peer >= p->code.k) return nullptr;
    if (len) *len = static_cast<size_t>(r->nunits) * kTile;
    return p->q[peer].get() + static_cast<size_t>(r->slot) * kTile;
}

// The staging of parity_lid's given residuals, acquired on its first use (a pool that sees
// no multi-loss request holds none), for another parity of a mask (checked).  NULL: no memory.
static Buf *pool_given_staging(cec_recovery_pool *p, int parity_lid) {
    Buf &g = p->given[parity_lid - p->code.k];
    const size_t bytes = static_cast<size_t>(p->book.capacity()) * kTile;
    if (!g && !g.acquire_mapped(p->device, bytes)) {
        (void)fail(CEC_ENOMEM, "recovery pool: %zu bytes of staging for parity %d's residuals", bytes, parity_lid);
        return nullptr;
    }
    return &g;
}

CEC_API uint8_t *cec_recovery_pool_parity_staging(cec_recovery_pool *p, int id, int parity_lid, size_t *len) {
    const poolbook::Req *r = pool_find(p, id);
    if (!r) {
        (void)fail(CEC_EINVAL, "cec_recovery_pool_parity_staging: request %d", id);
        return nullptr;
    }
    // only where add_residual would take one: another parity of a multi-loss request's mask
    // (given already or not) -- nothing is acquired for any other lid or request
    if (const poolbook::Refusal why = p->book.check_residual(id, parity_lid); why && why != poolbook::kTwice) {
        (void)fail(CEC_EINVAL, "cec_recovery_pool_parity_staging: request %d takes no residual of lid %d", id,
                   parity_lid);
        return nullptr;
    }
    Buf *g = pool_given_staging(p, parity_lid);
    if (!g) return nullptr;
    if (len) *len = static_cast<size_t>(r->nunits) * kTile;
    return g->get() + static_cast<size_t>(r->slot) * kTile;
}

static const char *const kResidualRefusal[] = {
    "accepted", "no such request", "the lid is no parity of the request's mask",
    "the pool's own parity (its residual is the pool's)", "that parity's residual was given before",
    "a single-loss request takes no residual", "a (request, parity) pair listed twice"};

// The n residuals into their stagings, then -- every copy done -- the bookkeeping: a failed
// device copy (CEC_EHIP) or staging allocation (CEC_ENOMEM) leaves nothing given or queued.
static int pool_give(cec_recovery_pool *p, const char *op, const int *ids, const int *lids,
                     const void *const *residuals, int n) {
    for (int i = 0; i < n; ++i) {
        const poolbook::Req &r = p->book.reqs[ids[i]];
        Buf *g = pool_given_staging(p, lids[i]);
        if (!g) return CEC_ENOMEM;
        const size_t off = static_cast<size_t>(r.slot) * kTile, len = static_cast<size_t>(r.nunits) * kTile;
        uint8_t *const dst = g->get() + off;
        if (residuals[i] == dst) {
            // received in place (cec_recovery_pool_parity_staging): nothing to copy
        } else if (const PtrKind kind = classify(residuals[i]); kind.known && !kind.host && kind.dev) {
            // device memory: one synchronous copy by the runtime per residual (host memory of
            // any kind: memcpy)
            int dev;
            if (int rc = current_device(&dev)) return rc;
            if (dev != p->device) return fail(CEC_EINVAL, "pool of device %d used on %d", p->device, dev);
            if (hipError_t e = hipMemcpy(dst, kind.dev, len, hipMemcpyDefault); e != hipSuccess) {
                (void)hipGetLastError();
                return fail(CEC_EHIP, "%s: copy of residual %d: %s", op, i, hipGetErrorString(e));
            }
        } else {
            memcpy(dst, residuals[i], len);
        }
    }
    // (a request's last residual may make it ready: the next flush looks)
    for (int i = 0; i < n; ++i) p->book.note_residual(ids[i], lids[i]);
    return CEC_OK;
}

CEC_API int cec_recovery_pool_add_residuals(cec_recovery_pool *p, const int *ids, const int *parity_lids,
                                            const void *const *residuals, int n) {
    if (!p || n < 0 || (n > 0 && (!ids || !parity_lids || !residuals)))
        return fail(CEC_EINVAL, "cec_recovery_pool_add_residuals: bad args");
    for (int i = 0; i < n; ++i)
        if (!residuals[i]) return fail(CEC_EINVAL, "cec_recovery_pool_add_residuals: residual %d is NULL", i);
    int bad = 0;
    if (poolbook::Refusal why = p->book.check_residuals(ids, parity_lids, n, &bad))
        return fail(CEC_EINVAL, "cec_recovery_pool_add_residuals: residual %d (request %d, parity %d): %s", bad,
                    ids[bad], parity_lids[bad], kResidualRefusal[why]);
    return pool_give(p, "cec_recovery_pool_add_residuals", ids, parity_lids, residuals, n);
}

CEC_API int cec_recovery_pool_add_residual(cec_recovery_pool *p, int id, int parity_lid, const void *residual) {
    if (!p || !residual) return fail(CEC_EINVAL, "cec_recovery_pool_add_residual: bad args");
    if (poolbook::Refusal why = p->book.check_residual(id, parity_lid))
        return fail(CEC_EINVAL, "cec_recovery_pool_add_residual: request %d, parity %d: %s", id, parity_lid,
                    kResidualRefusal[why]);
    return pool_give(p, "cec_recovery_pool_add_residual", &id, &parity_lid, &residual, 1);
}

CEC_API int cec_recovery_pool_ready(const cec_recovery_pool *p, int id) { return p && p->book.ready(id) ? 1 : 0; }

static int pool_out_host(cec_recovery_pool *p, int planes) {  // the _host solves' output planes, on first use
    const size_t bytes = static_cast<size_t>(p->book.capacity()) * kTile;
    for (int x = 0; x < planes; ++x)
        if (!p->out[x] && !p->out[x].acquire_mapped(p->device, bytes))
            return fail(CEC_ENOMEM, "recovery pool: %zu bytes of host output (plane %d)", bytes, x);
    return CEC_OK;
}

// The streams of a flush.  Its patterns outlive the call (PoolTables is append-only) with
// the slots baked in, so the slots are a function of (k, m) alone, the same in every flush:
// poolbook::FlushSlots states the layout and its bound (42 of kMaxStreams = 48 at k = 16,
// m = 8), and this fills it in that order.  A buffer not acquired yet leaves its slot empty;
// no pattern of the launch names it (launch_combine checks).
struct FlushStreams {
    Streams st;
    poolbook::FlushSlots at;
    FlushStreams(const cec_recovery_pool *p, uint8_t *const *o, bool to_host) : at{p->code.k, p->code.m} {
        const int k = p->code.k, m = p->code.m;
        bool ok = st.add(p->parity) == at.parity() && st.add(p->residual.get()) == at.residual();
        for (int j = 0; j < k; ++j) ok &= st.add(p->q[j].alias()) == at.reply(j);
        for (int j = 0; j < k; ++j)  // arenas by data lid, or host planes by lost ordinal
            ok &= st.add(to_host ? (j < CEC_MAX_M && p->out[j] ? p->out[j].alias() : nullptr) : o ? o[j] : nullptr) ==
                  at.out(j);
        for (int q = 0; q < m; ++q) ok &= st.add(p->given[q] ? p->given[q].alias() : nullptr) == at.given(k + q);
        if (!ok || st.n != at.count()) st.refused = true;  // (the layout and this constructor disagree)
    }
};

// One combination that rebuilds the n lost shards of `mask` from C[self] = sum_i a[i] *
// (input i of c, i < n_self: R itself, or the inputs of a flush's R') and the given
// residuals, which it adds as inputs from the slots given_slot(parity lid):
//   shard x = sum_p inv[x][p] * C[p]      (memcached.c:7907-7922; exact in GF(2^8))
// into out_slot(x, lost lid), slot-addressed if by_src.  Appends n outputs to c.
template <class GivenSlot, class OutSlot>
static int pool_solve_combo(const cec_recovery_pool *p, uint32_t mask, Combo &c, const int *a, int n_self,
                            GivenSlot given_slot, OutSlot out_slot, bool by_src) {
    Loss ls;
    if (int rc = Loss::of(p->code, mask, "recovery pool", &ls)) return rc;
    const int self = ls.index_of_parity(p->book.self);
    if (self < 0) return fail(CEC_EINVAL, "recovery pool: mask 0x%x does not name this parity", mask);
    int in_given[CEC_MAX_M];
    for (int r = 0; r < ls.n; ++r)
        if (r != self) in_given[r] = c.in(given_slot(ls.pars[r]), true);
    for (int x = 0; x < ls.n; ++x) {
        Combo::Out &q = c.out(out_slot(x, ls.lost[x]), kModeWrite, by_src);
        for (int i = 0; i < n_self; ++i) q.coef[i] = gf_mul(ls.at(x, self), a[i]);
        for (int r = 0; r < ls.n; ++r)
            if (r != self) q.coef[in_given[r]] = ls.at(x, r);
    }
    return CEC_OK;
}

// The pool's mapped diff staging, grown to hold `len` bytes (idle: every earlier call
// completed before returning).
static int pool_diff_staging(cec_recovery_pool *p, size_t len, const char *op) {
    if (p->diff.bytes() < len && !p->diff.acquire_mapped(p->device, std::max<size_t>(len, size_t(1) << 20)))
        return fail(CEC_ENOMEM, "%s: %zu bytes of diff staging", op, len);
    return CEC_OK;
}

static int pool_solve_run(cec_recovery_pool *p, int dev, std::vector<int> ids, uint8_t *const *out, bool to_host,
                          hipStream_t s);

static uint32_t pool_arenas(uint8_t *const *out, int k) {  // the data lids with an output arena, as the book's bit set
    uint32_t have = 0;
    for (int j = 0; j < k && out; ++j) have |= out[j] ? 1u << j : 0;
    return have;
}

// Fold every queued reply in one launch.  With `out` (k arenas by data lid) or to_host (the
// host planes at the request's slots instead of out[lost]), a request that this flush makes
// ready is solved in the same pass, from the same inputs (exact in GF(2^8), as
// cec_recovery_finish).  Returns the requests solved, or for a pass that solves none, folded.
static int pool_flush(cec_recovery_pool *p, uint8_t *const *out, bool to_host, void *stream) {
    const std::vector<int> &queued = p->book.queued_ids;
    if (queued.empty()) return 0;
    int dev;
    if (int rc = current_device(&dev)) return rc;
    if (dev != p->device) return fail(CEC_EINVAL, "pool of device %d used on %d", p->device, dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    UseNote note_{p->uses, s};
    const int k = p->code.k;
    poolbook::Plan plan = p->book.plan_flush(out || to_host, to_host, pool_arenas(out, k));
    if (int rc = pool_out_host(p, plan.planes)) return rc;  // (none unless to_host)
    const FlushStreams fs(p, out, to_host);
    const int engine = op_engine(false);
    if (p->tables.engine != engine) {  // the table's coefficient form is per engine
        p->tables.reset(dev, engine);
        p->flush_pat.clear();
    }
    // one pattern per poolbook::flush_key, from the pool's persistent table
    std::vector<char> used;
    size_t nt = 0;
    int folded = 0;
    for (size_t x = 0; x < queued.size(); ++x) {
        if (plan.action[x] == poolbook::kNothing) continue;
        const poolbook::Req &r = p->book.reqs[queued[x]];
        const bool fused = plan.action[x] == poolbook::kFused, folds = r.queued || r.touch_pending;
        const uint64_t key = poolbook::flush_key(r.queued, r.touch_pending, fused, r.mask, to_host);
        auto it = p->flush_pat.find(key);
        if (it == p->flush_pat.end()) {
            Combo c;
            // R' = sum_i a[i] * input i.  P, arena-addressed: the first-touch copy
            // (recovery.c:79-82); else R itself, slot-addressed
            int a[kPatN] = {};
            a[r.touch_pending ? c.in(fs.at.parity()) : c.in(fs.at.residual(), true)] = 1;
            for (int j = 0; j < k; ++j)
                if (r.queued & (1u << j)) a[c.in(fs.at.reply(j), true)] = p->code.at(p->book.self, j);  // recovery.c:91-93
            const int n_self = c.n_in;  // (<= k - n + 1; the given residuals make it at most k)
            if (folds) {  // (a residual-only pass leaves R as it is)
                Combo::Out &o = c.out(fs.at.residual(), kModeWrite, true);
                for (int i = 0; i < n_self; ++i) o.coef[i] = a[i];
            }
            if (fused) {  // the leader's bottom half in the same pass (memcached.c:7907-7922)
                // host plane x, slot-addressed; or the lost lid's arena, arena offset
                if (int rc = pool_solve_combo(
                        p, r.mask, c, a, n_self, [&](int lid) { return fs.at.given(lid); },
                        [&](int ord, int lid) { return fs.at.out(to_host ? ord : lid); }, to_host))
                    return rc;
            }
            // (<= 4 outputs: one pattern; refused before the table or the key map change)
            const int at = static_cast<int>(p->tables.pats.size());
            if (int rc = build_patterns({c}, 0, engine, p->tables.pats, p->tables.rows, true)) return rc;
            it = p->flush_pat.emplace(key, at).first;
        }
        used.resize(p->tables.pats.size(), 0);
        used[it->second] = 1;
        if (nt + r.nunits > static_cast<size_t>(p->book.capacity()))  // (cannot happen: the queue holds an id once)
            return fail(CEC_EINVAL, "recovery pool: a flush of more units than the tile buffer; not launched");
        nt += append_tiles(p->tiles.get<Tile>() + nt, static_cast<uint64_t>(r.ub) * kTile,
                           static_cast<uint64_t>(r.slot) * kTile, static_cast<uint32_t>(r.nunits) * kTile,
                           static_cast<uint32_t>(it->second));
        folded += r.queued != 0;  // (not one only solved by this pass, nor a first touch without a reply)
    }
    if (nt) {
        used.resize(p->tables.pats.size(), 0);
        if (int rc = p->tables.sync(s)) return rc;
        // (the pool's tile buffer: whole 4 KiB units on 4 KiB offsets)
        if (int rc = launch_combine(dev, fs.st,
                                    Tables{p->tables.d.get(), p->tables.cap_pats, p->tables.pats.data(), &used},
                                    nullptr, launch_shape(p->tables.pats, &used), engine == CEC_ENGINE_LDS,
                                    TileSource::whole_units(p->tiles.alias<Tile>(), nt), s, false))
            return rc;
        // tile buffer and staging reusable; rebuilt shards visible if out is host memory
        if (int rc = stream_wait(s, to_host || (out && any_host_memory(out, k)))) return rc;
    }
    const int n_solved = p->book.commit_flush(plan, to_host) + static_cast<int>(plan.later.size());
    // Four losses and more: R' is in HBM and the launch above is complete (the tile buffer is
    // free again), so the solve reads the new R as an explicit solve would -- the hazard of
    // cec_recovery_finish's R' (an output over an input of a split combination) does not arise.
    if (!plan.later.empty())
        if (int rc = pool_solve_run(p, dev, std::move(plan.later), out, to_host, s)) return rc;
    return out || to_host ? n_solved : folded;
}

CEC_API int cec_recovery_pool_flush(cec_recovery_pool *p, void *stream) {
    if (!p) return fail(CEC_EINVAL, "cec_recovery_pool_flush: pool is NULL");
    return pool_flush(p, nullptr, false, stream);
}

CEC_API int cec_recovery_pool_flush_solve(cec_recovery_pool *p, uint8_t *const *out, void *stream) {
    if (!p || !out) return fail(CEC_EINVAL, "cec_recovery_pool_flush_solve: bad args");
    return pool_flush(p, out, false, stream);
}

CEC_API int cec_recovery_pool_flush_solve_host(cec_recovery_pool *p, void *stream) {
    if (!p) return fail(CEC_EINVAL, "cec_recovery_pool_flush_solve_host: pool is NULL");
    return pool_flush(p, nullptr, true, stream);
}

CEC_API const uint8_t *cec_recovery_pool_output_lost(const cec_recovery_pool *p, int id, int x, size_t *len) {
    const poolbook::Req *r = pool_find(p, id);
    if (!r || !r->solved || !r->solved_host || x < 0 || x >= p->book.n_lost(r->mask) || !p->out[x]) return nullptr;
    if (len) *len = static_cast<size_t>(r->nunits) * kTile;
    return p->out[x].get() + static_cast<size_t>(r->slot) * kTile;
}

CEC_API const uint8_t *cec_recovery_pool_output(const cec_recovery_pool *p, int id, size_t *len) {
    return cec_recovery_pool_output_lost(p, id, 0, len);
}

CEC_API int cec_recovery_pool_solved(const cec_recovery_pool *p, int id) {
    const poolbook::Req *r = pool_find(p, id);
    return r && r->solved ? 1 : 0;
}

CEC_API int cec_recovery_pool_complete(const cec_recovery_pool *p, int id) { return p && p->book.complete(id) ? 1 : 0; }

CEC_API int cec_recovery_pool_fold_update(cec_recovery_pool *p, int peer, uint64_t addr, const void *diff,
                                          uint32_t len, void *stream) {
    if (!p || (len && !diff) || peer < 0 || peer >= p->code.k)
        return fail(CEC_EINVAL, "cec_recovery_pool_fold_update: bad args");
    if (len == 0) return 0;
    int dev;
    if (int rc = current_device(&dev)) return rc;
    if (dev != p->device) return fail(CEC_EINVAL, "pool of device %d used on %d", p->device, dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    UseNote note_{p->uses, s};
    if (int rc = cec_recovery_pool_flush(p, stream); rc < 0) return rc;
    // tiles: the update's pieces, slot-addressed (R) and diff-addressed (src_off); at most
    // one tile per unit, so they fit the pool's tile buffer
    std::vector<poolbook::Piece> pieces;
    const int units = p->book.pieces(p->book.touched_spans(), addr, len, peer, 0, pieces);
    size_t nt = 0;
    for (const poolbook::Piece &pc : pieces)  // (a lost lid's diff after the solve: R moved on)
        nt += append_tiles(p->tiles.get<Tile>() + nt, pc.r_off, pc.d_off, pc.len, 0);
    if (nt == 0) return 0;
    const uint8_t *d = static_cast<const uint8_t *>(device_view_of(diff));
    if (!d) {  // pageable diff: through the pool's mapped pinned staging (zero-copy)
        if (int rc = pool_diff_staging(p, len, "cec_recovery_pool_fold_update")) return rc;
        memcpy(p->diff.get(), diff, len);
        d = p->diff.alias();
    }
    const Fold f = fold(p->code, p->book.self, d, p->residual.get(), peer);  // recovery.c:123
    if (int rc = run_combos(dev, f.st, f.combos, TileSource::window(p->tiles.alias<Tile>(), p->tiles.get<Tile>(), nt), s))
        return rc;
    if (int rc = stream_wait(s, false)) return rc;  // (the residual is in HBM)
    return units;
}

// recovery_try_update_unit for a whole drain window (u[0..n), host buffers, any data
// lids): the same rule as cec_recovery_pool_fold_update per update, every fold of the
// window in one upload and one launch per overlap wave.  The pieces are packed into the
// pool's mapped diff staging; pieces of different updates that meet in R go to separate
// waves (colour_intervals over the tiles sorted by R offset: XOR folds commute, so any
// order within a byte gives the sequential bytes).  units[i] (optional) = the units update i
// folded, as cec_recovery_pool_fold_update returns them.
CEC_API int cec_recovery_pool_fold_updates(cec_recovery_pool *p, const cec_host_update *u, int n, int *units,
                                           void *stream) {
    if (!p || n < 0 || (n > 0 && !u)) return fail(CEC_EINVAL, "cec_recovery_pool_fold_updates: bad args");
    for (int i = 0; i < n; ++i)
        if (u[i].src_lid >= static_cast<uint32_t>(p->code.k) || (u[i].len && !u[i].buf))
            return fail(CEC_EINVAL, "cec_recovery_pool_fold_updates: update %d (lid %u)", i, u[i].src_lid);
    if (units)
        for (int i = 0; i < n; ++i) units[i] = 0;
    if (n == 0) return 0;
    int dev;
    if (int rc = current_device(&dev)) return rc;
    if (dev != p->device) return fail(CEC_EINVAL, "pool of device %d used on %d", p->device, dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    UseNote note_{p->uses, s};
    if (int rc = cec_recovery_pool_flush(p, stream); rc < 0) return rc;
    const std::vector<poolbook::Span> spans = p->book.touched_spans();
    std::vector<poolbook::Piece> pieces;
    int total_units = 0;
    for (int i = 0; i < n && !spans.empty(); ++i) {
        const int nu = p->book.pieces(spans, u[i].addr, u[i].len, static_cast<int>(u[i].src_lid), i, pieces);
        total_units += nu;
        if (units) units[i] = nu;
    }
    size_t staged = 0;
    for (const poolbook::Piece &pc : pieces) staged += pc.len;
    if (pieces.empty()) return 0;
    if (int rc = pool_diff_staging(p, staged, "cec_recovery_pool_fold_updates")) return rc;
    // tiles (one per unit piece: R offsets are unit-aligned per slot), packed pieces
    std::vector<Tile> tiles;
    tiles.reserve(pieces.size() + staged / kTile + 1);
    size_t so = 0;
    for (const poolbook::Piece &pc : pieces) {
        memcpy(p->diff.get() + so, static_cast<const uint8_t *>(u[pc.upd].buf) + pc.d_off, pc.len);
        Tile tmp[33];
        for (uint32_t o = 0; o < pc.len;) {  // <= 32 units per step: <= 33 tiles (append_tiles' split)
            const uint32_t step = std::min<uint32_t>(pc.len - o, 32 * kTile);
            const size_t nt = append_tiles(tmp, pc.r_off + o, so + o, step, u[pc.upd].src_lid);
            tiles.insert(tiles.end(), tmp, tmp + nt);
            o += step;
        }
        so += pc.len;
    }
    // waves: greedy colouring of the tiles by R offset
    std::sort(tiles.begin(), tiles.end(), [](const Tile &x, const Tile &y) { return x.off < y.off; });
    const size_t nt = tiles.size();
    std::vector<int> wave_of(nt);
    const size_t nw = colour_intervals(
        nt, [&](size_t t) { return std::pair<uint64_t, uint64_t>(tiles[t].off, tiles[t].off + tiles[t].len); },
        [&](size_t t, int w) { wave_of[t] = w; });
    std::vector<size_t> at(nw + 1, 0);  // counting sort by wave (stable)
    for (int w : wave_of) ++at[w + 1];
    for (size_t w = 0; w < nw; ++w) at[w + 1] += at[w];
    std::vector<size_t> order(nt);
    for (size_t t = 0; t < nt; ++t) order[at[wave_of[t]]++] = t;
    // the tile buffer: the pool's own, or for a window wider than it, a cached one
    Buf wide;
    const Buf &tb = nt <= static_cast<size_t>(p->book.capacity()) ? p->tiles : wide;
    if (&tb == &wide && !wide.acquire_mapped(dev, nt * sizeof(Tile)))
        return fail(CEC_ENOMEM, "cec_recovery_pool_fold_updates: %zu tiles", nt);
    WaveTiles wt(tb.get<Tile>());
    for (size_t t : order) {
        wt.enter(wave_of[t]);
        wt.add(tiles[t].off, tiles[t].src_off, tiles[t].len, tiles[t].pattern);  // (one tile each, as cut above)
    }
    // the packed diff pieces into R; pattern index = the update's data lid (recovery.c:123)
    const Fold f = fold(p->code, p->book.self, p->diff.alias(), p->residual.get());
    std::vector<char> used(p->code.k, 0);
    for (const poolbook::Piece &pc : pieces) used[u[pc.upd].src_lid] = 1;
    // an earlier wave may still read the diff staging and the tiles (the pool's own or `wide`,
    // which goes back to the cache after the guard), which the next call overwrites from the host
    InFlight guard(s);
    for (int w = 0; w < wt.waves(); ++w)
        if (int rc = run_combos(dev, f.st, f.combos, wt.window(w, tb.alias<Tile>()), s, &used)) return rc;
    if (int rc = stream_wait(s, false)) return rc;  // (the residual is in HBM; staging and tiles reusable)
    guard.dismiss();
    return total_units;
}

// The solve of checked requests (live, ready, distinct, their outputs there), the flush done:
// ceil(n_max / 4) launches for the largest loss count among them.
//   to_host: plane x [slot] instead of out[lost_x][off].
// The first k combinations are the single losses, one per lost data lid x (out[x] = inv * R,
// pattern index = x), always all k of them: one table per pool and engine in the coefficient
// cache, whatever the mix of single-loss requests (`used` picks the kernel shape).  Each
// multi-loss mask listed adds one combination behind them.  The requests are listed by
// descending loss count, so launch g (outputs 4g .. 4g+3) runs over a prefix of the tile
// buffer: those that lose more than 4g shards.
static int pool_solve_run(cec_recovery_pool *p, int dev, std::vector<int> ids, uint8_t *const *out, bool to_host,
                          hipStream_t s) {
    const int k = p->code.k;
    const poolbook::Book &book = p->book;
    auto losses = [&](int id) { return book.n_lost(book.reqs[id].mask); };
    auto only_lost = [&](int id) { return __builtin_ctz(book.lost_lids(book.reqs[id].mask)); };  // of a single loss
    std::stable_sort(ids.begin(), ids.end(), [&](int a, int b) { return losses(a) > losses(b); });
    const int n_max = losses(ids.front());
    if (int rc = pool_out_host(p, to_host ? n_max : 0)) return rc;
    Streams st;
    const int s_residual = st.add(p->residual.get());
    int s_plane[CEC_MAX_M], s_given[CEC_MAX_M], s_arena[CEC_MAX_K];
    std::fill(s_plane, s_plane + CEC_MAX_M, -1);
    std::fill(s_given, s_given + CEC_MAX_M, -1);
    if (to_host) s_plane[0] = st.add(p->out[0].alias());
    for (int x = 0; x < k && !to_host; ++x) s_arena[x] = st.add(out[x]);
    std::vector<Combo> combos(k);
    for (int x = 0; x < k; ++x) {
        Combo &c = combos[x];
        const int in_r = c.in(s_residual, true);  // R, slot-addressed
        // plane 0, slot-addressed; or the lost lid's arena, arena offset
        Combo::Out &o = to_host ? c.out(s_plane[0], kModeWrite, true) : c.out(s_arena[x], kModeWrite);
        const int cx = p->code.at(p->book.self, x);
        o.coef[in_r] = cx ? gf_inv(cx) : 0;  // memcached.c:7907-7922, n_lost = 1
    }
    std::map<uint32_t, int> combo_of;  // multi-loss mask -> its combination
    size_t nt = 0;
    std::vector<size_t> tiles_upto(poolbook::solve_launches(n_max), 0);  // launch g's prefix of the tiles
    for (int id : ids) {
        const poolbook::Req &r = book.reqs[id];
        const int n = losses(id);
        int pattern;
        if (n == 1) {
            pattern = only_lost(id);
        } else {
            auto it = combo_of.find(r.mask);
            if (it == combo_of.end()) {
                Combo c;
                const int one = 1;
                c.in(s_residual, true);  // C[self] = R, slot-addressed
                if (int rc = pool_solve_combo(
                        p, r.mask, c, &one, 1,
                        [&](int lid) {  // (given: checked ready)
                            int &slot = s_given[lid - k];
                            return slot >= 0 ? slot : (slot = st.add(p->given[lid - k].alias()));
                        },
                        [&](int ord, int lid) {
                            if (!to_host) return s_arena[lid];
                            return s_plane[ord] >= 0 ? s_plane[ord] : (s_plane[ord] = st.add(p->out[ord].alias()));
                        },
                        to_host))
                    return rc;
                it = combo_of.emplace(r.mask, static_cast<int>(combos.size())).first;
                combos.push_back(c);
            }
            pattern = it->second;
        }
        if (nt + r.nunits > static_cast<size_t>(p->book.capacity()))  // (cannot happen once ids are distinct)
            return fail(CEC_EINVAL, "cec_recovery_pool_solve: more units than the tile buffer");
        nt += append_tiles(p->tiles.get<Tile>() + nt, static_cast<uint64_t>(r.ub) * kTile,
                           static_cast<uint64_t>(r.slot) * kTile, static_cast<uint32_t>(r.nunits) * kTile,
                           static_cast<uint32_t>(pattern));
        for (int g = 0; g < poolbook::solve_launches(n); ++g) tiles_upto[g] = nt;
    }
    const int engine = op_engine(false);
    for (size_t g = 0; g < tiles_upto.size(); ++g) {
        // the combinations launch g's tiles name: those listed that have an output past 4g
        std::vector<char> used(combos.size(), 0);
        for (int id : ids) {
            if (losses(id) == 1) {
                used[only_lost(id)] = g == 0;
            } else if (losses(id) > static_cast<int>(g) * kPatL) {
                used[combo_of[book.reqs[id].mask]] = 1;
            }
        }
        std::vector<Pattern> pats;
        std::vector<uint8_t> rows;
        if (int rc = build_patterns(combos, g, engine, pats, rows)) return rc;
        // (whole 4 KiB units on 4 KiB offsets, as the flush's)
        if (int rc = run_combine(dev, st, pats, rows, TileSource::whole_units(p->tiles.alias<Tile>(), tiles_upto[g]), s,
                                 &used, engine))
            return rc;
    }
    if (int rc = stream_wait(s, to_host || any_host_memory(out, k))) return rc;
    p->book.mark_solved(ids, to_host);
    return CEC_OK;
}

static int pool_solve(cec_recovery_pool *p, const int *ids, int n, uint8_t *const *out, bool to_host,
                      void *stream) {
    if (!p || n < 0 || (n > 0 && (!ids || (!out && !to_host))))
        return fail(CEC_EINVAL, "cec_recovery_pool_solve: bad args");
    if (n == 0) return CEC_OK;
    int dev;
    if (int rc = current_device(&dev)) return rc;
    if (dev != p->device) return fail(CEC_EINVAL, "pool of device %d used on %d", p->device, dev);
    if (int rc = cec_recovery_pool_flush(p, stream); rc < 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    UseNote note_{p->uses, s};
    int x = 0;
    const uint32_t arenas = pool_arenas(out, p->code.k);
    switch (p->book.check_solve(ids, n, to_host, arenas, &x)) {
    case poolbook::kAccepted: break;
    case poolbook::kIncomplete:
        return fail(CEC_EINVAL, "cec_recovery_pool_solve: request %d missing or incomplete", ids[x]);
    case poolbook::kListedTwice: return fail(CEC_EINVAL, "cec_recovery_pool_solve: request %d listed twice", ids[x]);
    case poolbook::kNotReady:
        return fail(CEC_EINVAL, "cec_recovery_pool_solve: request %d loses %d shards and not every other "
                                "participating parity's residual has been given (cec_recovery_pool_add_residual)",
                    ids[x], p->book.n_lost(p->book.reqs[ids[x]].mask));
    default:
        return fail(CEC_EINVAL, "cec_recovery_pool_solve: out[%d] is NULL",
                    __builtin_ctz(p->book.lost_lids(p->book.reqs[ids[x]].mask) & ~arenas));
    }
    return pool_solve_run(p, dev, std::vector<int>(ids, ids + n), out, to_host, s);
}

CEC_API int cec_recovery_pool_solve(cec_recovery_pool *p, const int *ids, int n, uint8_t *const *out,
                                    void *stream) {
    return pool_solve(p, ids, n, out, false, stream);
}

CEC_API int cec_recovery_pool_solve_host(cec_recovery_pool *p, const int *ids, int n, void *stream) {
    return pool_solve(p, ids, n, nullptr, true, stream);
}

CEC_API int cec_recovery_pool_residual(cec_recovery_pool *p, int id, void *dst, void *stream) {
    const poolbook::Req *r = pool_find(p, id);
    if (!r || !dst) return fail(CEC_EINVAL, "cec_recovery_pool_residual: request %d / dst", id);
    // no reply ever queued (a mask without data lids is touched from begin): R[slot] holds what
    // the slots' previous owner left, and check_solve refuses such a request too
    if (!r->touched) return fail(CEC_EINVAL, "cec_recovery_pool_residual: request %d holds no residual yet", id);
    if (int rc = cec_recovery_pool_flush(p, stream); rc < 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    UseNote note_{p->uses, s};
    HIP_TRY(hipMemcpyAsync(dst, p->residual.get() + static_cast<size_t>(r->slot) * kTile,
                           static_cast<size_t>(r->nunits) * kTile, hipMemcpyDefault, s));
    HIP_TRY(hipStreamSynchronize(s));
    return CEC_OK;
}

CEC_API int cec_recovery_pool_end(cec_recovery_pool *p, int id) {
    const poolbook::Req *r = pool_find(p, id);
    if (!r) return fail(CEC_EINVAL, "cec_recovery_pool_end: request %d", id);
    // a reply still queued: fold it first, it may share a tile list
    if (int rc = r->queued ? cec_recovery_pool_flush(p, nullptr) : 0; rc < 0) return rc;
    p->book.end(id);  // (also out of the queue, where a residual since the last flush left it)
    return CEC_OK;
}

CEC_API int cec_recovery_pool_active(const cec_recovery_pool *p) { return p ? p->book.active() : 0; }
