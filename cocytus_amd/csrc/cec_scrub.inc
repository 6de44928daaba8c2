// cec_scrub.inc -- device parity check: locate and repair bad 4 KiB units.
// Included by cec_runtime.hip; not a separate TU.  scrub_launch is built from the parts
// launch_combine is: a TileSource to walk, a planner of cec_launchplan.hpp (plan_scrub) and
// enqueue_launch.  Only the kernel and its argument block differ.
//
// Where the server would call it: the idle loop (idle_event_handler,
// memcached.c:5712-5734) walks the arenas in idle time, and after a CEC_EHIP from
// cec_drainer_apply / cec_recovery_pool_fold_updates (some waves applied, a retry would
// apply them twice) a scrub over the window's ranges tells which units of the parity
// arena are now wrong, instead of stopping the process.  All k + m arenas of the group
// must sit on this device (DESIGN.md §3's placement).
//   * cec_scrub: clear the report (one memset), one scrub_kernel launch per group of up
//     to four parities (cec_kernels.hpp: reads all streams, writes nothing to the arenas;
//     a clean wave touches the report not at all), copy the counter back.  PERM engine.
//   * cec_scrub_findings: the per-tile words come back only when the counter is non-zero;
//     each flagged word is classified on the host (cec_scrub_classify).
//   * cec_scrub_repair: no new kernel -- one cec_decode over the tiles of located data lids
//     (one mask per lost lid), one cec_encode per located parity.

namespace {

constexpr uint32_t kScrubHead = 4;  // words before the per-tile words: [0] the counter (16-B aligned words)

template <int NT, int LT, bool kExact>
void launch_scrub_k(const ScrubArgs &a, const LaunchPlan &lp, hipStream_t s) {
    hipLaunchKernelGGL((scrub_kernel<NT, LT, kExact>), dim3(lp.grid), dim3(lp.block), lp.lds_bytes, s, a);
}

// The kernel of a planned launch: `exact` (scrub_exact) one of the three compiled for the
// codes the suite uses, else the plan's rung of the capacity ladder.
void launch_scrub(bool exact, const ScrubArgs &a, const LaunchPlan &lp, hipStream_t s) {
    if (exact && lp.nt == 3) return launch_scrub_k<3, 2, true>(a, lp, s);
    if (exact && lp.nt == 4) return launch_scrub_k<4, 2, true>(a, lp, s);
    if (exact) return launch_scrub_k<6, 3, true>(a, lp, s);
#define CEC_SG(NT, LT)                           \
    launch_scrub_k<NT, LT, false>(a, lp, s);    \
    return;
    CEC_CAPACITY_RUNGS_FROM_4(lp.nt, lp.lt, CEC_SG)
#undef CEC_SG
}

}  // namespace

static_assert(CEC_KERNEL_SCRUB == 3, "cec_launch_record::kind");

struct cec_scrub_report {
    int device = -1;
    uint64_t max_tiles = 0;
    Buf d_mem, h_mem;           // device words and their pinned mirror (cec_cache.inc), viewed as:
    uint32_t *d_buf = nullptr;  // kScrubHead + max_tiles words: counter, then one word per tile
    uint32_t *h_buf = nullptr;  // pinned mirror, same layout
    Tracker uses;
    // the last run
    bool valid = false;     // a run was enqueued in full (else wait / findings / repair refuse)
    bool waited = false;    // ... and its stream synchronised: count holds
    bool fetched = false;   // ... and the words copied back
    hipStream_t stream = nullptr;
    const cec_plan *plan = nullptr;  // must outlive findings / repair (tile offsets)
    uint64_t implicit_len = 0;
    uint64_t n_tiles = 0;
    int64_t count = 0;
    int k = 0, m = 0;
    std::vector<int> matrix;
};

CEC_API int cec_scrub_create(cec_scrub_report **out, uint64_t max_tiles) {
    if (!out) return fail(CEC_EINVAL, "cec_scrub_create: out is NULL");
    *out = nullptr;
    if (max_tiles < 1 || max_tiles > kScrubMaxTiles)
        return fail(CEC_EINVAL, "cec_scrub_create: max_tiles %llu outside [1, %llu] (one dispatch)",
                    static_cast<unsigned long long>(max_tiles), static_cast<unsigned long long>(kScrubMaxTiles));
    int dev;
    if (int r = current_device(&dev)) return r;
    cec_scrub_report *s = new (std::nothrow) cec_scrub_report;
    if (!s) return fail(CEC_ENOMEM, "cec_scrub_create: host allocation");
    s->device = dev;
    s->max_tiles = max_tiles;
    const size_t bytes = sizeof(uint32_t) * (kScrubHead + max_tiles);
    if (!s->d_mem.acquire(dev_cache(), dev, bytes) || !s->h_mem.acquire(pin_cache(), dev, bytes)) {
        delete s;
        return fail(CEC_ENOMEM, "cec_scrub_create: %zu bytes of report", bytes);
    }
    s->d_buf = s->d_mem.get<uint32_t>();
    s->h_buf = s->h_mem.get<uint32_t>();
    *out = s;
    return CEC_OK;
}

CEC_API int cec_scrub_destroy(cec_scrub_report *s) {
    if (!s) return CEC_OK;
    (void)s->uses.wait(s->device);  // its own runs, not the device
    delete s;  // (its buffers go back to the caches)
    return CEC_OK;
}

CEC_API int cec_scrub_release_stream(cec_scrub_report *s, void *stream) {
    if (!s) return fail(CEC_EINVAL, "cec_scrub_release_stream: report is NULL");
    if (hipError_t e = s->uses.release(s->device, static_cast<hipStream_t>(stream)); e != hipSuccess)
        return fail(CEC_EHIP, "cec_scrub_release_stream: %s", hipGetErrorString(e));
    return CEC_OK;
}

// The two patterns of one launch over parities [p0, p0 + lt) of the code, for the arena
// scrub and for the digest check (cec_digest.inc) alike:
// [0]: the syndrome's coefficients; [1]: ratio[q][j] = MATRIX(k+p0+q, j) / MATRIX(k+p0, j)
// as PERM tables (a zero denominator leaves the zero table: lid j is then ruled out
// wherever S_q is non-zero, which errs towards UNLOCATED)
static std::vector<Pattern> scrub_patterns(const Code &code, int p0, int lt) {
    const int k = code.k;
    std::vector<Pattern> pats(2, blank_pattern());
    Pattern &c = pats[0], &r = pats[1];
    c.n_in = r.n_in = k;
    c.n_out = r.n_out = lt;
    for (int j = 0; j < k; ++j) c.in_stream[j] = r.in_stream[j] = j;
    for (int l = 0; l < lt; ++l) {
        c.out_stream[l] = r.out_stream[l] = k + l;
        c.out_mode[l] = r.out_mode[l] = kModeXor;
        for (int j = 0; j < k; ++j) {
            set_coef(c, l, j, code.at(k + p0 + l, j), CEC_ENGINE_PERM);
            const int den = code.at(k + p0, j);
            set_coef(r, l, j, l && den ? gf_div(code.at(k + p0 + l, j), den) : 0, CEC_ENGINE_PERM);
        }
    }
    return pats;
}

// One launch: parities [p0, p0 + lt) of the code against the k data streams.
static int scrub_launch(int dev, cec_scrub_report *s, int k, int m, const int *matrix, const uint8_t *const *data,
                        const uint8_t *const *parity, int p0, int lt, const TileSource &src, hipStream_t stream) {
    const std::vector<Pattern> pats = scrub_patterns(Code{k, m, matrix}, p0, lt);
    const bool whole_code = p0 == 0 && lt == m;
    ScrubArgs a;
    memset(&a, 0, sizeof a);
    uintptr_t bases_or = 0;
    for (int i = 0; i < k + lt; ++i) {
        a.base[i] = i < k ? data[i] : parity[p0 + i - k];
        bases_or |= reinterpret_cast<uintptr_t>(a.base[i]);
    }
    a.tiles = src.tiles;
    a.implicit_len = src.implicit_len;
    a.words = s->d_buf + kScrubHead;
    a.counter = s->d_buf;
    a.n_tiles = static_cast<uint32_t>(src.n_tiles);
    a.syn_shift = static_cast<uint32_t>(p0);
    Launch l;
    l.plan = plan_scrub(k, lt, whole_code, src.n_tiles, src.n_line_tiles, bases_or, g_knobs, waves_per_cu_cap(),
                        g_dev[dev].lds_per_cu);
    l.tb = Tables{nullptr, pats.size(), pats.data(), nullptr};
    l.bases = a.base;
    l.en = k;
    l.el = lt;
    l.uses[0] = src.uses;
    l.uses[1] = &s->uses;
    return enqueue_launch(dev, stream, l, [&](const LaunchPlan &lp, const uint8_t *d) {
        a.pattern = reinterpret_cast<const Pattern *>(d);
        a.split_shift = lp.split_shift;
        a.grid = lp.grid;
        launch_scrub(scrub_exact(k, lt, whole_code), a, lp, stream);
        return CEC_OK;
    });
}

// One launch of the digest check (cec_digest.inc), with scrub_launch's arguments.
static int digest_check_launch(int dev, cec_scrub_report *s, int k, int m, const int *matrix,
                               const uint8_t *const *data, const uint8_t *const *parity, int p0, int lt,
                               const TileSource &src, hipStream_t stream);

// cec_scrub and cec_scrub_digests: clear the report, one launch per four parities, copy
// the counter back.  `digests`: data / parity are the group's digest arrays (32 B per tile)
// and the launches are digest_check_launch's; the plan or len then only counts the tiles
// and gives each finding its off / len.
static int scrub_common(const char *op, bool digests, cec_scrub_report *s, int k, int m, const int *matrix,
                        const uint8_t *const *data, const uint8_t *const *parity, const cec_plan *plan, uint64_t len,
                        void *stream_) {
    const char *what = digests ? " digests" : "";
    if (int r = check_code(k, m, matrix)) return r;
    if (!data || !parity) return fail(CEC_EINVAL, "%s: NULL %s array", op, digests ? "digest" : "arena");
    for (int j = 0; j < k; ++j)
        if (!data[j]) return fail(CEC_EINVAL, "%s: data%s[%d] is NULL", op, what, j);
    for (int p = 0; p < m; ++p)
        if (!parity[p])
            return fail(CEC_EINVAL, "%s: parity%s[%d] is NULL (a lost parity cannot be checked)", op, what, p);
    if (digests) {
        if (!s) {  // no report can exist without a device: say that first (CEC_ENODEV)
            int none;
            if (int r = current_device(&none)) return r;
        }
        for (int i = 0; i < k + m; ++i)
            if (reinterpret_cast<uintptr_t>(i < k ? data[i] : parity[i - k]) & 15)
                return fail(CEC_EINVAL, "%s: digest array of lid %d is not 16-byte aligned", op, i);
    }
    if (!s) return fail(CEC_EINVAL, "%s: report is NULL", op);
    const uint64_t n_tiles = plan ? static_cast<uint64_t>(plan->n_tiles) : (len + kTile - 1) / kTile;
    if (n_tiles > s->max_tiles)
        return fail(CEC_EINVAL, "%s: %llu tiles, the report holds %llu", op,
                    static_cast<unsigned long long>(n_tiles), static_cast<unsigned long long>(s->max_tiles));
    int dev;
    if (int r = current_device(&dev)) return r;
    if (s->device != dev) return fail(CEC_EINVAL, "report built on device %d used on device %d", s->device, dev);
    TileSource src;
    if (int r = plan ? TileSource::of_plan(plan, dev, &src) : TileSource::of_region(len, &src)) return r;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    s->valid = s->waited = s->fetched = false;  // until this run is enqueued in full
    t_last_engine = CEC_ENGINE_PERM;            // whatever cec_set_engine says
    s->uses.note(stream);
    HIP_TRY(hipMemsetAsync(s->d_buf, 0, sizeof(uint32_t) * (kScrubHead + n_tiles), stream));
    if (n_tiles)
        for (int p0 = 0; p0 < m; p0 += kPatL)
            if (int r = (digests ? digest_check_launch : scrub_launch)(dev, s, k, m, matrix, data, parity, p0,
                                                                       std::min<int>(kPatL, m - p0), src, stream))
                return r;
    HIP_TRY(hipMemcpyAsync(s->h_buf, s->d_buf, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    s->stream = stream;
    s->plan = plan;
    s->implicit_len = len;
    s->n_tiles = n_tiles;
    s->k = k;
    s->m = m;
    s->matrix.assign(matrix, matrix + (k + m) * k);
    s->valid = true;
    return CEC_OK;
}

CEC_API int cec_scrub(cec_scrub_report *s, int k, int m, const int *matrix, const uint8_t *const *data,
                      const uint8_t *const *parity, const cec_plan *plan, void *stream) {
    if (!plan) return fail(CEC_EINVAL, "cec_scrub: plan is NULL");
    if (int r = single_pattern_plan(plan, "cec_scrub")) return r;
    return scrub_common("cec_scrub", false, s, k, m, matrix, data, parity, plan, 0, stream);
}

CEC_API int cec_scrub_region(cec_scrub_report *s, int k, int m, const int *matrix, const uint8_t *const *data,
                             const uint8_t *const *parity, size_t len, void *stream) {
    return scrub_common("cec_scrub", false, s, k, m, matrix, data, parity, nullptr, len, stream);
}

CEC_API int64_t cec_scrub_wait(cec_scrub_report *s) {
    if (!s || !s->valid) return fail(CEC_EINVAL, "cec_scrub_wait: no successful run to wait for");
    if (!s->waited) {
        if (hipError_t e = hipStreamSynchronize(s->stream); e != hipSuccess) {
            (void)hipGetLastError();
            s->valid = false;
            return fail(CEC_EHIP, "cec_scrub_wait: %s", hipGetErrorString(e));
        }
        s->count = static_cast<int64_t>(__atomic_load_n(s->h_buf, __ATOMIC_ACQUIRE));
        s->waited = true;
    }
    return s->count;
}

CEC_API int cec_scrub_classify(uint32_t word, int k, int m, const int *matrix) {
    if (int r = check_code(k, m, matrix)) return r;
    const uint32_t syn = word & 0xFFu, ruled = (word >> 8) & 0xFFFFu;
    if (syn == 0 || (syn >> m) != 0)
        return fail(CEC_EINVAL, "cec_scrub_classify: word 0x%x has no syndrome bit of the code's %d", word, m);
    g_err[0] = 0;  // (CEC_SCRUB_UNLOCATED is a verdict, not an error: no message)
    if (m < 2) return CEC_SCRUB_UNLOCATED;
    if (__builtin_popcount(syn) == 1) return k + __builtin_ctz(syn);
    int lid = CEC_SCRUB_UNLOCATED;
    for (int j = 0; j < k; ++j) {
        if (ruled & (1u << j)) continue;
        if (lid != CEC_SCRUB_UNLOCATED) return CEC_SCRUB_UNLOCATED;  // two candidates
        lid = j;
    }
    if (lid == CEC_SCRUB_UNLOCATED) return lid;
    uint32_t expect = 0;  // the parities lid j reaches: all m for an MDS matrix
    for (int p = 0; p < m; ++p) expect |= (Code{k, m, matrix}.at(k + p, lid) ? 1u : 0u) << p;
    return syn == expect ? lid : CEC_SCRUB_UNLOCATED;
}

// Wait, and bring the words back if any tile is flagged.
static int scrub_fetch(cec_scrub_report *s, const char *op) {
    if (!s || !s->valid) return fail(CEC_EINVAL, "%s: no successful run to report", op);
    const int64_t n = cec_scrub_wait(s);
    if (n < 0) return static_cast<int>(n);
    if (n > 0 && !s->fetched) {
        HIP_TRY(hipMemcpyAsync(s->h_buf + kScrubHead, s->d_buf + kScrubHead, sizeof(uint32_t) * s->n_tiles,
                               hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        s->fetched = true;
    }
    return CEC_OK;
}

static Tile scrub_tile(const cec_scrub_report *s, uint64_t t) {
    if (s->plan) return s->plan->h_tiles[t];
    const uint64_t o = t * kTile;
    return Tile{o, o, static_cast<uint32_t>(std::min<uint64_t>(kTile, s->implicit_len - o)), 0};
}

CEC_API int cec_scrub_findings(cec_scrub_report *s, cec_scrub_finding *out, int cap) {
    if (cap < 0 || (cap > 0 && !out)) return fail(CEC_EINVAL, "cec_scrub_findings: bad args");
    if (int r = scrub_fetch(s, "cec_scrub_findings")) return r;
    if (s->count == 0) return 0;
    const uint32_t *words = s->h_buf + kScrubHead;
    int n = 0;
    for (uint64_t t = 0; t < s->n_tiles && n < cap; ++t) {
        if (!(words[t] & 0xFFu)) continue;
        const Tile tl = scrub_tile(s, t);
        cec_scrub_finding &f = out[n++];
        f.tile = t;
        f.off = tl.off;
        f.len = tl.len;
        f.syndromes = words[t] & 0xFFu;
        f.ruled_out = (words[t] >> 8) & 0xFFFFu;
        f.lid = cec_scrub_classify(words[t], s->k, s->m, s->matrix.data());
    }
    return n;
}

CEC_API int cec_scrub_repair(cec_scrub_report *s, int k, int m, const int *matrix, uint8_t *const *data,
                             uint8_t *const *parity, void *stream, int *unrepaired) {
    if (int r = check_code(k, m, matrix)) return r;
    if (!data || !parity || !unrepaired) return fail(CEC_EINVAL, "cec_scrub_repair: NULL argument");
    for (int j = 0; j < k; ++j)
        if (!data[j]) return fail(CEC_EINVAL, "cec_scrub_repair: data[%d] is NULL", j);
    for (int p = 0; p < m; ++p)
        if (!parity[p]) return fail(CEC_EINVAL, "cec_scrub_repair: parity[%d] is NULL", p);
    if (int r = scrub_fetch(s, "cec_scrub_repair")) return r;
    if (k != s->k || m != s->m || memcmp(matrix, s->matrix.data(), sizeof(int) * (k + m) * k) != 0)
        return fail(CEC_EINVAL, "cec_scrub_repair: not the code of the report's last run");
    *unrepaired = 0;
    if (s->count == 0) return CEC_OK;
    // located data lids: one decode, one mask per lost lid (every lid but j, led by the
    // first parity); located parities: one encode each
    std::vector<cec_extent> dext, pext[CEC_MAX_M];
    std::vector<uint32_t> masks;
    int mask_of[CEC_MAX_K];
    for (int &x : mask_of) x = -1;
    const uint32_t *words = s->h_buf + kScrubHead;
    for (uint64_t t = 0; t < s->n_tiles; ++t) {
        if (!(words[t] & 0xFFu)) continue;
        const int lid = cec_scrub_classify(words[t], k, m, matrix);
        const Tile tl = scrub_tile(s, t);
        if (lid < 0) {
            ++*unrepaired;
        } else if (lid < k) {
            if (mask_of[lid] < 0) {
                int connected[CEC_MAX_K + CEC_MAX_M];
                for (int i = 0; i < k + m; ++i) connected[i] = i != lid;
                mask_of[lid] = static_cast<int>(masks.size());
                masks.push_back(cec_recovery_mask(k, m, k, connected));
            }
            dext.push_back(cec_extent{tl.off, tl.off, tl.len, static_cast<uint32_t>(mask_of[lid])});
        } else {
            pext[lid - k].push_back(cec_extent{tl.off, tl.off, tl.len, 0});
        }
    }
    const uint8_t *arenas[CEC_MAX_K + CEC_MAX_M];
    for (int j = 0; j < k; ++j) arenas[j] = data[j];
    for (int p = 0; p < m; ++p) arenas[k + p] = parity[p];
    int rc = CEC_OK;
    if (!dext.empty()) {
        cec_plan *pl = nullptr;
        if (int r = cec_plan_create(&pl, dext.data(), static_cast<int>(dext.size()), stream)) return r;
        // out[j] is the data arena itself: j is not among its own decode's inputs
        rc = cec_decode(k, m, matrix, masks.data(), static_cast<int>(masks.size()), arenas, data, pl, stream);
        const int rd = cec_plan_destroy(pl);  // (waits for the decode: a repair is rare)
        if (rc == CEC_OK) rc = rd;
    }
    for (int p = 0; p < m && rc == CEC_OK; ++p) {
        if (pext[p].empty()) continue;
        uint8_t *only[CEC_MAX_M] = {};
        only[p] = parity[p];
        cec_plan *pl = nullptr;
        if (int r = cec_plan_create(&pl, pext[p].data(), static_cast<int>(pext[p].size()), stream)) return r;
        rc = cec_encode(k, m, matrix, arenas, only, pl, stream);
        const int rd = cec_plan_destroy(pl);
        if (rc == CEC_OK) rc = rd;
    }
    return rc;
}
