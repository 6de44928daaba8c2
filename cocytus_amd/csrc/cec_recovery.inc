// cec_recovery.inc -- online recovery over 4 KiB unit ranges (SURVEY §8f rank 2).
// Included by cec_runtime.hip after cec_drain.inc (shares the launch internals); not a
// separate TU.  HostStager takes PackPool / split_copy from cec_hostplan.hpp and Buf /
// HalfPipe from cec_cache.inc, where device_view_of and any_host_memory (classify) live too.
//
// A cec_recovery is one recovery request on a participating parity
// (recovery_queue_item, recovery.h:57-69).  The residual of the whole unit range lives
// in HBM; every byte of arithmetic is a combine-kernel launch over the range:
//   add_peer (recovery_recover_units, recovery.c:61-96): first peer
//       R = P[range] ^ c*D   (first-touch copy of the parity units fused in),
//     later peers R ^= c*D, c = M[self][peer];
//     a mask that names no data lid (k <= m) has no peer: create makes R = P[range] itself;
//   fold_update (recovery_try_update_unit, recovery.c:99-131): R[piece] ^= c*diff
//     while the range is touched and the peer has not contributed;
//   solve (complete_recovery_bottom_half, memcached.c:7842-7922): out = inv * C.
// The reference keeps these flags per 4 KiB unit; a session's peers always deliver the
// whole range at once (recover_units_reply, memcached.c:4277-4281), so the per-unit
// flags are uniform over the range and are kept once per session.

namespace {

// Host <-> device copies of pageable buffers through two pinned halves: the pack pool
// copies chunk i into one half while the DMA of chunk i-1 (other half) runs.
class HostStager {
  public:
    ~HostStager() { (void)pipe_.wait_all(); }  // (then the pinned halves go back to the cache)
    int init(int dev, size_t chunk) {
        chunk_ = chunk;
        // pinning pages costs milliseconds per 32 MiB: sessions share the pinned cache
        if (!pinned_.acquire(pin_cache(), dev, 2 * chunk_) || pipe_.create(hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            return fail(CEC_ENOMEM, "pinned staging of 2 x %zu bytes", chunk_);
        }
        pool_.reset(new PackPool(pack_threads() - 1));
        return CEC_OK;
    }
    void pcopy(uint8_t *dst, const uint8_t *src, size_t len) {
        const CopyItem one{dst, src, len};
        split_copy(pool_.get(), &one, 1, size_t(1) << 20);
    }
    // Host -> device; the copies are enqueued on s (complete in stream order).
    int upload(uint8_t *ddst, const uint8_t *hsrc, size_t len, hipStream_t s) {
        for (size_t o = 0; o < len; o += chunk_) {
            const size_t n = std::min(chunk_, len - o);
            HIP_TRY(pipe_.wait(h_));
            uint8_t *pin = pinned_.get() + h_ * chunk_;
            pcopy(pin, hsrc + o, n);
            HIP_TRY(hipMemcpyAsync(ddst + o, pin, n, hipMemcpyHostToDevice, s));
            HIP_TRY(pipe_.record(h_, s));
            h_ ^= 1;
        }
        return CEC_OK;
    }
    // Device -> host; synchronous (hdst holds the bytes on return).
    int download(uint8_t *hdst, const uint8_t *dsrc, size_t len, hipStream_t s) {
        size_t prev_off = 0, prev_n = 0;
        int prev_h = -1;
        for (size_t o = 0; o < len; o += chunk_) {
            const size_t n = std::min(chunk_, len - o);
            HIP_TRY(pipe_.wait(h_));
            HIP_TRY(hipMemcpyAsync(pinned_.get() + h_ * chunk_, dsrc + o, n, hipMemcpyDeviceToHost, s));
            HIP_TRY(pipe_.record(h_, s));
            if (prev_h >= 0) {  // drain the previous chunk while this one is in flight
                HIP_TRY(pipe_.wait(prev_h));
                pcopy(hdst + prev_off, pinned_.get() + prev_h * chunk_, prev_n);
            }
            prev_h = h_;
            prev_off = o;
            prev_n = n;
            h_ ^= 1;
        }
        if (prev_h >= 0) {
            HIP_TRY(pipe_.wait(prev_h));
            pcopy(hdst + prev_off, pinned_.get() + prev_h * chunk_, prev_n);
        }
        return CEC_OK;
    }

  private:
    size_t chunk_ = 0;
    Buf pinned_;  // 2 x chunk_
    HalfPipe pipe_;
    int h_ = 0;
    std::unique_ptr<PackPool> pool_;
};

}  // namespace

struct cec_recovery {
    int device = -1;
    int lid_self = 0;
    std::vector<int> matrix;
    Code code;  // over `matrix`
    uint32_t mask = 0;
    int ub = 0, ue = 0;
    uint64_t base = 0, nbuf = 0;   // arena offset and bytes of the unit range
    const uint8_t *parity = nullptr;  // this parity's arena + base
    uint8_t *residual = nullptr, *scratch = nullptr;  // device, nbuf each
    bool touched = false;
    uint32_t contributed = 0;
    Tracker uses;  // the streams of its calls (destroy waits for those only)
    HostStager stager;
};


CEC_API int cec_recovery_destroy(cec_recovery *r) {
    if (!r) return CEC_OK;
    (void)r->uses.wait(r->device);  // the session's own calls only (nothing if none was made)
    dev_cache().release(r->device, r->residual, r->nbuf);
    dev_cache().release(r->device, r->scratch, r->nbuf);
    delete r;
    return CEC_OK;
}

CEC_API int cec_recovery_release_stream(cec_recovery *r, void *stream) {
    if (!r) return fail(CEC_EINVAL, "cec_recovery_release_stream: session is NULL");
    if (hipError_t e = r->uses.release(r->device, static_cast<hipStream_t>(stream)); e != hipSuccess)
        return fail(CEC_EHIP, "cec_recovery_release_stream: %s", hipGetErrorString(e));
    return CEC_OK;
}

// A mask that names no data lid (k <= m: k parities rebuild all k shards) has no peer whose
// reply would bring the first touch about: R = P[range] (recovery.c:79-82, no fold behind it)
// in one launch on s, complete on return.  From then on the session is touched, so every
// later diff is folded into R as into any touched range.
static int recovery_touch_alone(cec_recovery *r, hipStream_t s) {
    UseNote note_{r->uses, s};
    Streams st;
    const int s_parity = st.add(r->parity), s_residual = st.add(r->residual);
    if (int rc = run_combos_region(r->device, st, {multiply_combo(1, false, s_parity, s_residual)}, r->nbuf, s))
        return rc;
    if (int rc = stream_wait(s, false)) return rc;  // (the residual is in HBM)
    r->touched = true;
    return CEC_OK;
}

CEC_API int cec_recovery_create(cec_recovery **out, int k, int m, const int *matrix, int lid_self,
                                uint32_t mask, int unit_begin, int unit_end,
                                const uint8_t *parity_arena, void *stream) {
    if (!out) return fail(CEC_EINVAL, "cec_recovery_create: out is NULL");
    *out = nullptr;
    if (int r = check_code(k, m, matrix)) return r;
    if (lid_self < k || lid_self >= k + m || !(mask & (1u << lid_self)) || !mask_ok(k, m, mask) ||
        unit_begin < 0 || unit_end < unit_begin || !parity_arena)
        return fail(CEC_EINVAL, "cec_recovery_create: bad lid %d / mask 0x%x / units [%d, %d]",
                    lid_self, mask, unit_begin, unit_end);
    int dev;
    if (int r = current_device(&dev)) return r;
    cec_recovery *s = new (std::nothrow) cec_recovery;
    if (!s) return fail(CEC_ENOMEM, "cec_recovery_create: host allocation");
    s->device = dev;
    s->lid_self = lid_self;
    s->code = Code::owned(s->matrix, k, m, matrix);
    s->mask = mask;
    s->ub = unit_begin;
    s->ue = unit_end;
    s->base = static_cast<uint64_t>(unit_begin) * kTile;
    s->nbuf = static_cast<uint64_t>(unit_end - unit_begin + 1) * kTile;
    s->parity = parity_arena + s->base;
    s->residual = static_cast<uint8_t *>(dev_cache().acquire(dev, s->nbuf));
    s->scratch = static_cast<uint8_t *>(dev_cache().acquire(dev, s->nbuf));
    if (!s->residual || !s->scratch) {
        cec_recovery_destroy(s);
        return fail(CEC_ENOMEM, "cec_recovery_create: 2 x %llu device bytes",
                    static_cast<unsigned long long>(s->nbuf));
    }
    if (int rc = s->stager.init(dev, std::min<uint64_t>(s->nbuf, uint64_t(16) << 20))) {
        cec_recovery_destroy(s);
        return rc;
    }
    if (!(mask & ((1u << k) - 1)))
        if (int rc = recovery_touch_alone(s, static_cast<hipStream_t>(stream))) {
            cec_recovery_destroy(s);
            return rc;
        }
    *out = s;
    return CEC_OK;
}

// Device view of a caller buffer of len bytes: in place if device-accessible, else
// staged into `scratch` (enqueued on s).
static int device_input(cec_recovery *r, const void *p, size_t len, uint8_t *scratch,
                        hipStream_t s, const uint8_t **dv) {
    if (void *v = device_view_of(p)) {
        *dv = static_cast<const uint8_t *>(v);
        return CEC_OK;
    }
    *dv = scratch;
    return r->stager.upload(scratch, static_cast<const uint8_t *>(p), len, s);
}

// Device scratch of `bytes` per buffer for one synchronous call, released to dev_cache()
// when the call returns -- after a stream sync, if any was taken: work enqueued on s may
// still read or write it.
struct DevScratch {
    int dev;
    size_t bytes;
    hipStream_t s;
    std::vector<uint8_t *> bufs = {};
    ~DevScratch() {
        if (!bufs.empty()) (void)hipStreamSynchronize(s);
        for (uint8_t *p : bufs) dev_cache().release(dev, p, bytes);
    }
    int take(const char *op, uint8_t **p) {
        if (!(*p = static_cast<uint8_t *>(dev_cache().acquire(dev, bytes))))
            return fail(CEC_ENOMEM, "%s: device scratch", op);
        bufs.push_back(*p);
        return CEC_OK;
    }
};

// The device view of the residual parity `lid` shipped (the whole range): in place, or, if
// pageable, staged into scratch of `tmp` (enqueued on s).
static int peer_residual(cec_recovery *r, const char *op, const void *const *peer_residuals, int lid,
                         DevScratch &tmp, hipStream_t s, const uint8_t **dv) {
    if (!peer_residuals || !peer_residuals[lid]) return fail(CEC_EINVAL, "%s: residual of parity %d missing", op, lid);
    uint8_t *stage = nullptr;
    if (!device_view_of(peer_residuals[lid]))
        if (int rc = tmp.take(op, &stage)) return rc;
    return device_input(r, peer_residuals[lid], r->nbuf, stage, s, dv);
}

CEC_API int cec_recovery_add_peer(cec_recovery *r, int peer, const void *units, void *stream) {
    if (!r || !units || peer < 0 || peer >= r->code.k || !(r->mask & (1u << peer)))
        return fail(CEC_EINVAL, "cec_recovery_add_peer: peer %d is not a data lid of the mask", peer);
    if (r->contributed & (1u << peer))
        return fail(CEC_EINVAL, "cec_recovery_add_peer: peer %d already applied (recovery.c:75)", peer);
    int dev;
    if (int rc = current_device(&dev)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    UseNote note_{r->uses, s};
    const uint8_t *d;
    if (int rc = device_input(r, units, r->nbuf, r->scratch, s, &d)) return rc;
    Streams st;
    const int s_units = st.add(d), s_residual = st.add(r->residual), s_parity = st.add(r->parity);
    Combo c;
    Combo::Out &o = c.out(s_residual, r->touched ? kModeXor : kModeWrite);
    o.coef[c.in(s_units)] = r->code.at(r->lid_self, peer);  // recovery.c:91-93
    if (!r->touched) o.coef[c.in(s_parity)] = 1;            // first touch: R = P ^ c*D (recovery.c:79-82 + 91)
    if (int rc = run_combos_region(dev, st, {c}, r->nbuf, s)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    r->touched = true;
    r->contributed |= 1u << peer;
    return CEC_OK;
}

CEC_API int cec_recovery_fold_update(cec_recovery *r, int peer, uint64_t addr, const void *diff,
                                     uint32_t len, void *stream) {
    if (!r || (len && !diff) || peer < 0 || peer >= r->code.k)
        return fail(CEC_EINVAL, "cec_recovery_fold_update: bad args");
    // recovery.c:116-119: units not touched yet pick the update up from the parity
    // arena at first touch; a peer that already contributed sent post-update bytes.
    if (!r->touched || (r->contributed & (1u << peer))) return 0;
    const uint64_t lo = std::max(addr, r->base), hi = std::min(addr + len, r->base + r->nbuf);
    if (lo >= hi) return 0;
    int dev;
    if (int rc = current_device(&dev)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    UseNote note_{r->uses, s};
    const uint8_t *piece = static_cast<const uint8_t *>(diff) + (lo - addr);
    const uint8_t *d;
    if (int rc = device_input(r, piece, hi - lo, r->scratch, s, &d)) return rc;
    if (int rc = cec_region_multiply(d, r->code.at(r->lid_self, peer), hi - lo, r->residual + (lo - r->base),
                                     1, s))
        return rc;
    if (int rc = stream_wait(s, false)) return rc;  // per-SET call: its latency is its cost (residual in HBM)
    return static_cast<int>((hi - 1) / kTile - lo / kTile + 1);
}

CEC_API int cec_recovery_complete(const cec_recovery *r) {
    if (!r) return 0;
    const uint32_t data = r->mask & ((1u << r->code.k) - 1);
    return (r->contributed & data) == data ? 1 : 0;
}

CEC_API const uint8_t *cec_recovery_residual(const cec_recovery *r) { return r ? r->residual : nullptr; }
CEC_API uint64_t cec_recovery_bytes(const cec_recovery *r) { return r ? r->nbuf : 0; }

CEC_API int cec_recovery_solve(cec_recovery *r, const void *const *peer_residuals, void *const *out,
                               void *stream) {
    if (!r || !out) return fail(CEC_EINVAL, "cec_recovery_solve: bad args");
    if (!cec_recovery_complete(r))
        return fail(CEC_EINVAL, "cec_recovery_solve: not every data peer of mask 0x%x applied", r->mask);
    int dev;
    if (int rc = current_device(&dev)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    UseNote note_{r->uses, s};
    Loss ls;
    if (int rc = Loss::of(r->code, r->mask, "cec_recovery_solve", &ls)) return rc;
    if (ls.n == 0) return CEC_OK;
    DevScratch tmp{r->device, r->nbuf, s};  // staged inputs / host outputs
    Streams st;
    Combo c;
    for (int j = 0; j < ls.n; ++j) {
        const uint8_t *cj = r->residual;
        if (ls.pars[j] != r->lid_self)
            if (int rc = peer_residual(r, "cec_recovery_solve", peer_residuals, ls.pars[j], tmp, s, &cj)) return rc;
        c.in(st.add(cj));
    }
    std::vector<std::pair<uint8_t *, uint8_t *>> downloads;  // (host dst, device src)
    for (int x = 0; x < ls.n; ++x) {
        void *o = out[ls.lost[x]];
        if (!o) return fail(CEC_EINVAL, "cec_recovery_solve: out[%d] is NULL", ls.lost[x]);
        uint8_t *dv = static_cast<uint8_t *>(device_view_of(o));
        if (!dv) {
            if (int rc = tmp.take("cec_recovery_solve", &dv)) return rc;
            downloads.emplace_back(static_cast<uint8_t *>(o), dv);
        }
        Combo::Out &q = c.out(st.add(dv), kModeWrite);  // data[i] = calloc, then += (memcached.c:7913-7922)
        for (int j = 0; j < ls.n; ++j) q.coef[j] = ls.at(x, j);
    }
    if (int rc = run_combos_region(dev, st, {c}, r->nbuf, s)) return rc;
    for (auto &dl : downloads)
        if (int rc = r->stager.download(dl.first, dl.second, r->nbuf, s)) return rc;
    // Synchronous (cocytus_ec.h): out, device or pinned, holds the rebuilt bytes on return,
    // and the caller may reuse its peer-residual buffers.
    // (the system-scope fence only when the kernel wrote host-visible memory directly)
    return stream_wait(s, any_host_memory(reinterpret_cast<uint8_t *const *>(out), r->code.k));
}

// The last data peer's fold (recovery_recover_units, recovery.c:61-96) and the leader
// solve (complete_recovery_bottom_half, memcached.c:7842-7922) in one pass per piece:
//   R'  = R_or_P ^ c * D                        (kept: cec_recovery_residual)
//   out = inv[x][self] * R' ^ sum_{j != self} inv[x][j] * C_j
//       = inv_s * R_or_P ^ (inv_s * c) * D ^ ...  (exact in GF(2^8))
// Device or pinned buffers are used in place: one launch up to three lost shards (1 + n
// outputs, kPatL a launch: ceil((n + 1) / 4) launches for n lost), in which the kernel reads
// the peer's bytes and writes the rebuilt bytes over PCIe in both directions at once.
// Pageable buffers take the two-step path (add_peer, then solve): their cost is the
// host copy through pinned staging, and a piecewise fused pipeline measured slower
// (21.9 vs 17.5 ms for 256 MiB) because it serialises the pack and unpack copies.
CEC_API int cec_recovery_finish(cec_recovery *r, int peer, const void *units,
                                const void *const *peer_residuals, void *const *out, void *stream) {
    if (!r || !units || !out || peer < 0 || peer >= r->code.k || !(r->mask & (1u << peer)))
        return fail(CEC_EINVAL, "cec_recovery_finish: peer %d is not a data lid of the mask", peer);
    if (r->contributed & (1u << peer))
        return fail(CEC_EINVAL, "cec_recovery_finish: peer %d already applied (recovery.c:75)", peer);
    const uint32_t data_lids = r->mask & ((1u << r->code.k) - 1);
    if (((r->contributed | (1u << peer)) & data_lids) != data_lids)
        return fail(CEC_EINVAL, "cec_recovery_finish: peer %d is not the last data peer of mask 0x%x",
                    peer, r->mask);
    int dev;
    if (int rc = current_device(&dev)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    UseNote note_{r->uses, s};
    Loss ls;
    if (int rc = Loss::of(r->code, r->mask, "cec_recovery_finish", &ls)) return rc;
    if (ls.n == 0) return cec_recovery_add_peer(r, peer, units, stream);  // nothing lost: the fold alone
    const int self = ls.index_of_parity(r->lid_self);
    bool pageable = device_view_of(units) == nullptr;
    for (int x = 0; x < ls.n; ++x) {
        if (!out[ls.lost[x]]) return fail(CEC_EINVAL, "cec_recovery_finish: out[%d] is NULL", ls.lost[x]);
        pageable |= device_view_of(out[ls.lost[x]]) == nullptr;
    }
    if (self < 0 || pageable) {  // not a leader solve, or host bytes to stage
        if (int rc = cec_recovery_add_peer(r, peer, units, stream)) return rc;
        return cec_recovery_solve(r, peer_residuals, out, stream);
    }
    DevScratch tmp{r->device, r->nbuf, s};
    // one combination: inputs D, R_or_P, C_j (j != self), the other participating parities'
    // residuals, staged whole (multi-loss only); outputs R', out_x
    const int c = r->code.at(r->lid_self, peer);
    Streams st;
    Combo cb;
    const int in_d = cb.in(st.add(device_view_of(units)));
    int in_res[CEC_MAX_M];  // the input that carries the residual of parity pars[j]
    in_res[self] = cb.in(st.add(r->touched ? r->residual : r->parity));
    for (int j = 0; j < ls.n; ++j) {
        if (j == self) continue;
        const uint8_t *cj;
        if (int rc = peer_residual(r, "cec_recovery_finish", peer_residuals, ls.pars[j], tmp, s, &cj)) return rc;
        in_res[j] = cb.in(st.add(cj));
    }
    for (int x = 0; x < ls.n; ++x) {
        // data[i] = calloc, then += (memcached.c:7913-7922)
        Combo::Out &q = cb.out(st.add(device_view_of(out[ls.lost[x]])), kModeWrite);
        q.coef[in_d] = gf_mul(ls.at(x, self), c);
        for (int j = 0; j < ls.n; ++j) q.coef[in_res[j]] = ls.at(x, j);
    }
    // R' is stated last: once touched it overwrites the input R, and past kPatL outputs the
    // combination runs as successive launches -- every rebuilt shard must have read R by then
    // (build_patterns: an output that overwrites an input of its combination goes last).
    Combo::Out &ro = cb.out(st.add(r->residual), kModeWrite);
    ro.coef[in_d] = c;
    ro.coef[in_res[self]] = 1;
    if (int rc = run_combos_region(dev, st, {cb}, r->nbuf, s)) return rc;
    // Synchronous (cocytus_ec.h): the rebuilt bytes are in out on return, and units /
    // peer residuals may be reused by the caller.
    if (int rc = stream_wait(s, any_host_memory(reinterpret_cast<uint8_t *const *>(out), r->code.k))) return rc;
    r->touched = true;
    r->contributed |= 1u << peer;
    return CEC_OK;
}
