// cec_digest.inc -- 32-byte linear unit digests, and the scrub over them.
// Included by cec_runtime.hip after cec_scrub.inc; not a separate TU.
//
// cec_scrub needs all k + m arenas of a group on one device; Cocytus runs one process per
// shard.  The code is linear over GF(2^8), and so is the digest (cec_kernels.hpp), so
// digest(parity_p) = sum_j MATRIX(k+p, j) * digest(data_j): each process digests its own
// arena (cec_digest, 32 B per 4 KiB unit), ships the digests, and the leader runs the
// scrub's syndrome and ratio test on them (cec_scrub_digests) into the same
// cec_scrub_report -- wait / findings / classify / repair are cec_scrub.inc's, unchanged.
// Live digests: a process keeps its digest array current instead of taking it anew --
// cec_digest_apply_diffs folds every applied diff into it (digest_update_launch, which the
// drainer of cec_drain.inc calls once per round), and cec_digest_verify_region compares it
// with a fresh one through the same check.  With the whole group on one device the SET path
// keeps them: cec_digest_set folds new ^ old of a batch into the digests of every arena the
// batch changes, and cec_diff_update_digests runs it ahead of cec_diff_update.
// Built from the library's parts: a TileSource to walk, the planners of cec_launchplan.hpp
// (plan_digest, plan_digest_update, plan_digest_set, plan_digest_check), scrub_patterns for the check's
// coefficients, enqueue_launch.

namespace {

template <int NT, int LT>
void launch_digest_check_k(const DigestCheckArgs &a, const LaunchPlan &lp, hipStream_t s) {
    hipLaunchKernelGGL((digest_check_kernel<NT, LT>), dim3(lp.grid), dim3(lp.block), 0, s, a);
}

// The plan's rung of the capacity ladder.
void launch_digest_check(const DigestCheckArgs &a, const LaunchPlan &lp, hipStream_t s) {
#define CEC_DC(NT, LT)                           \
    launch_digest_check_k<NT, LT>(a, lp, s);    \
    return;
    CEC_CAPACITY_RUNGS_FROM_4(lp.nt, lp.lt, CEC_DC)
#undef CEC_DC
}

}  // namespace

static_assert(CEC_DIGEST_BYTES == kDigestBytes, "digest size");
static_assert(CEC_KERNEL_DIGEST == 4 && CEC_KERNEL_DIGEST_CHECK == 5 && CEC_KERNEL_DIGEST_UPDATE == 6 &&
                  CEC_KERNEL_DIGEST_SET == 7, "cec_launch_record::kind");
static_assert(CEC_MAX_K <= kPatN && CEC_MAX_M <= 2 * kPatL, "digest_set_kernel: data slots, two patterns of parities");
static_assert(CEC_MAX_K + CEC_MAX_M == kDigestArenas && kDigestArenas == kScrubStreams, "a whole group per launch");

static int digest_common(const char *op, int n, const uint8_t *const *arenas, uint8_t *const *digests,
                         const cec_plan *plan, uint64_t len, void *stream_) {
    if (!arenas || !digests) return fail(CEC_EINVAL, "%s: NULL arena or digest array", op);
    if (n < 1 || n > kDigestArenas) return fail(CEC_EINVAL, "%s: n = %d outside [1, %d]", op, n, kDigestArenas);
    for (int i = 0; i < n; ++i) {
        if (!arenas[i]) return fail(CEC_EINVAL, "%s: arenas[%d] is NULL", op, i);
        if (!digests[i]) return fail(CEC_EINVAL, "%s: digests[%d] is NULL", op, i);
        if (reinterpret_cast<uintptr_t>(digests[i]) & 15)
            return fail(CEC_EINVAL, "%s: digests[%d] is not 16-byte aligned", op, i);
    }
    int dev;
    if (int r = current_device(&dev)) return r;
    TileSource src;
    if (int r = plan ? TileSource::of_plan(plan, dev, &src) : TileSource::of_region(len, &src)) return r;
    t_last_engine = CEC_ENGINE_PERM;  // whatever cec_set_engine says
    Launch l;
    l.plan = plan_digest(n, src.n_tiles, g_knobs);
    if (l.plan.refusal == kPlanNothing) return CEC_OK;  // (before the fail hook counts)
    if (l.plan.refusal == kPlanTooLarge)
        return fail(CEC_EINVAL, "%s: %llu tiles x %d arenas, one launch holds %llu (tile, arena) pairs", op,
                    static_cast<unsigned long long>(src.n_tiles), n, static_cast<unsigned long long>(kDigestMaxWork));
    l.uses[0] = src.uses;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return enqueue_launch(dev, stream, l, [&](const LaunchPlan &lp, const uint8_t *) {
        DigestArgs a;
        memset(&a, 0, sizeof a);
        for (int i = 0; i < n; ++i) {
            a.base[i] = arenas[i];
            a.out[i] = digests[i];
        }
        a.tiles = src.tiles;
        a.implicit_len = src.implicit_len;
        a.n_tiles = static_cast<uint32_t>(src.n_tiles);
        a.n = static_cast<uint32_t>(n);
        a.n_work = a.n_tiles * a.n;  // (<= kDigestMaxWork)
        a.waves_shift = g_knobs.digest_waves_shift;
        hipLaunchKernelGGL(digest_kernel, dim3(lp.grid), dim3(lp.block), 0, stream, a);
        return CEC_OK;
    });
}

CEC_API int cec_digest(int n, const uint8_t *const *arenas, uint8_t *const *digests, const cec_plan *plan,
                       void *stream) {
    if (!plan) return fail(CEC_EINVAL, "cec_digest: plan is NULL");
    if (int r = single_pattern_plan(plan, "cec_digest")) return r;
    return digest_common("cec_digest", n, arenas, digests, plan, 0, stream);
}

CEC_API int cec_digest_region(int n, const uint8_t *const *arenas, uint8_t *const *digests, size_t len,
                              void *stream) {
    return digest_common("cec_digest_region", n, arenas, digests, nullptr, len, stream);
}

// The end of a live digest array of n_units units, as an arena offset.
static int digest_limit(const char *op, uint64_t n_units, uint64_t *limit) {
    if (n_units > (UINT64_MAX >> 12)) return fail(CEC_EINVAL, "%s: n_units %llu is no unit count", op,
                                                  static_cast<unsigned long long>(n_units));
    *limit = n_units * kTile;
    return CEC_OK;
}

// One digest_update_kernel launch: every tile of `src` (arena offset, src_off into `diffs`,
// pattern = source data lid) folded into the live digests of lid_self, which the caller has
// checked to hold every tile's unit.  One wave per tile, four per workgroup.
static int digest_update_launch(int dev, const Code &code, int lid_self, const uint8_t *diffs, uint8_t *digests,
                                const TileSource &src, hipStream_t stream) {
    Launch l;
    l.plan = plan_digest_update(src.n_tiles);
    if (l.plan.refusal == kPlanTooLarge)
        return fail(CEC_EINVAL, "digest update: %llu tiles, one launch holds %llu",
                    static_cast<unsigned long long>(src.n_tiles), static_cast<unsigned long long>(kDigestMaxWork));
    Pattern pat = blank_pattern();
    pat.n_in = code.k;
    pat.n_out = 1;
    for (int j = 0; j < code.k; ++j) set_coef(pat, 0, j, code.at(lid_self, j), CEC_ENGINE_PERM);
    l.tb = Tables{nullptr, 1, &pat, nullptr};
    l.uses[0] = src.uses;
    return enqueue_launch(dev, stream, l, [&](const LaunchPlan &lp, const uint8_t *d) {
        DigestUpdateArgs a;
        memset(&a, 0, sizeof a);
        a.diffs = diffs;
        a.digests = digests;
        a.tiles = src.tiles;
        a.pattern = reinterpret_cast<const Pattern *>(d);
        a.n_tiles = static_cast<uint32_t>(src.n_tiles);
        hipLaunchKernelGGL(digest_update_kernel, dim3(lp.grid), dim3(lp.block), 0, stream, a);
        return CEC_OK;
    });
}

CEC_API int cec_digest_apply_diffs(int k, int m, const int *matrix, int lid_self, const uint8_t *diffs,
                                   uint8_t *digests, uint64_t n_units, const cec_plan *plan, void *stream) {
    const char *op = "cec_digest_apply_diffs";
    if (int r = check_code(k, m, matrix)) return r;
    if (lid_self < 0 || lid_self >= k + m) return fail(CEC_EINVAL, "%s: lid_self %d outside [0, %d)", op, lid_self, k + m);
    if (!diffs || !digests || !plan) return fail(CEC_EINVAL, "%s: NULL diffs, digests or plan", op);
    if (reinterpret_cast<uintptr_t>(digests) & 15) return fail(CEC_EINVAL, "%s: digests is not 16-byte aligned", op);
    if (plan->n_ext && plan->max_pattern >= static_cast<uint32_t>(k))
        return fail(CEC_EINVAL, "%s: an extent names source shard %u (k = %d)", op, plan->max_pattern, k);
    uint64_t limit;
    if (int r = digest_limit(op, n_units, &limit)) return r;
    if (plan->max_end_ext >= 0 && plan->max_end > limit)
        return fail(CEC_EINVAL, "%s: extent %d ends at %llu, beyond n_units * 4096 = %llu", op, plan->max_end_ext,
                    static_cast<unsigned long long>(plan->max_end), static_cast<unsigned long long>(limit));
    int dev;
    if (int r = current_device(&dev)) return r;
    TileSource src;
    if (int r = TileSource::of_plan(plan, dev, &src)) return r;
    t_last_engine = CEC_ENGINE_PERM;  // whatever cec_set_engine says
    if (src.n_tiles == 0) return CEC_OK;
    return digest_update_launch(dev, Code{k, m, matrix}, lid_self, diffs, digests, src, static_cast<hipStream_t>(stream));
}

// What a digest-set launch needs, checked: made by digest_set_prepare and by nothing else.
struct DigestSet {
    int dev = 0;
    TileSource src;
    LaunchPlan plan;
    std::vector<Pattern> pats;  // one per four parities: coef / tab[p % 4][j] = MATRIX(k + p, j)
    DigestSetArgs args;         // all but `patterns`, which the enqueue fills
};

// Every check of cec_digest_set, and its plan: nothing is launched.  A NULL array of
// pointers, or a NULL entry, is an array that is not kept.
static int digest_set_prepare(const char *op, int k, int m, const int *matrix, const uint8_t *const *data,
                              const uint8_t *staging, uint8_t *const *data_digests, uint8_t *const *parity_digests,
                              uint64_t n_units, const cec_plan *plan, DigestSet *out) {
    if (int r = check_code(k, m, matrix)) return r;
    if (!data || !staging || !plan) return fail(CEC_EINVAL, "%s: NULL data, staging or plan", op);
    DigestSetArgs &a = out->args;
    memset(&a, 0, sizeof a);
    for (int j = 0; j < k; ++j) {
        if (!data[j]) return fail(CEC_EINVAL, "%s: data[%d] is NULL", op, j);
        a.data[j] = data[j];
    }
    for (int i = 0; i < k + m; ++i) {
        uint8_t *d = i < k ? (data_digests ? data_digests[i] : nullptr) : (parity_digests ? parity_digests[i - k] : nullptr);
        if (reinterpret_cast<uintptr_t>(d) & 15)
            return fail(CEC_EINVAL, "%s: %s_digests[%d] is not 16-byte aligned", op, i < k ? "data" : "parity",
                        i < k ? i : i - k);
        a.digests[i] = d;
    }
    if (plan->overlap) return fail(CEC_EOVERLAP, "%s: plan extents overlap (the op reads the old bytes)", op);
    if (plan->n_ext && plan->max_pattern >= static_cast<uint32_t>(k))
        return fail(CEC_EINVAL, "%s: an extent names source shard %u (k = %d)", op, plan->max_pattern, k);
    uint64_t limit;
    if (int r = digest_limit(op, n_units, &limit)) return r;
    if (plan->max_end_ext >= 0 && plan->max_end > limit)
        return fail(CEC_EINVAL, "%s: extent %d ends at %llu, beyond n_units * 4096 = %llu", op, plan->max_end_ext,
                    static_cast<unsigned long long>(plan->max_end), static_cast<unsigned long long>(limit));
    if (int r = current_device(&out->dev)) return r;
    if (int r = TileSource::of_plan(plan, out->dev, &out->src)) return r;
    out->plan = plan_digest_set(out->src.n_tiles);
    if (out->plan.refusal == kPlanTooLarge)
        return fail(CEC_EINVAL, "%s: %llu tiles, one launch holds %llu", op,
                    static_cast<unsigned long long>(out->src.n_tiles), static_cast<unsigned long long>(kDigestMaxWork));
    const Code code{k, m, matrix};
    out->pats.assign((m + kPatL - 1) / kPatL, blank_pattern());
    for (int p = 0; p < m; ++p) {
        Pattern &pat = out->pats[p / kPatL];
        pat.n_in = k;
        pat.n_out = p % kPatL + 1;
        for (int j = 0; j < k; ++j) set_coef(pat, p % kPatL, j, code.at(k + p, j), CEC_ENGINE_PERM);
    }
    a.staging = staging;
    a.tiles = out->src.tiles;
    a.n_tiles = static_cast<uint32_t>(out->src.n_tiles);  // (<= kDigestMaxWork)
    a.k = static_cast<uint32_t>(k);
    a.m = static_cast<uint32_t>(m);
    return CEC_OK;
}

// One digest_set_kernel launch of a prepared DigestSet (an empty plan: none).
static int digest_set_launch(const DigestSet &ds, hipStream_t stream) {
    t_last_engine = CEC_ENGINE_PERM;  // whatever cec_set_engine says
    if (ds.plan.refusal == kPlanNothing) return CEC_OK;  // (before the fail hook counts)
    Launch l;
    l.plan = ds.plan;
    l.tb = Tables{nullptr, ds.pats.size(), ds.pats.data(), nullptr};
    l.uses[0] = ds.src.uses;
    return enqueue_launch(ds.dev, stream, l, [&](const LaunchPlan &lp, const uint8_t *d) {
        DigestSetArgs a = ds.args;
        a.patterns = reinterpret_cast<const Pattern *>(d);
        hipLaunchKernelGGL(digest_set_kernel, dim3(lp.grid), dim3(lp.block), 0, stream, a);
        return CEC_OK;
    });
}

CEC_API int cec_digest_set(int k, int m, const int *matrix, const uint8_t *const *data, const uint8_t *staging,
                           uint8_t *const *data_digests, uint8_t *const *parity_digests, uint64_t n_units,
                           const cec_plan *plan, void *stream) {
    DigestSet ds;
    if (int r = digest_set_prepare("cec_digest_set", k, m, matrix, data, staging, data_digests, parity_digests,
                                   n_units, plan, &ds))
        return r;
    return digest_set_launch(ds, static_cast<hipStream_t>(stream));
}

CEC_API int cec_diff_update_digests(int k, int m, const int *matrix, uint8_t *const *data, const uint8_t *staging,
                                    uint8_t *const *parity, int install, uint8_t *const *data_digests,
                                    uint8_t *const *parity_digests, uint64_t n_units, const cec_plan *plan,
                                    void *stream) {
    const char *op = "cec_diff_update_digests";
    if (int r = check_code(k, m, matrix)) return r;
    if (!plan || !data || !staging || !parity) return fail(CEC_EINVAL, "%s: NULL data, staging, parity or plan", op);
    // strict about the arrays: every arena the op writes has its digests kept
    if (install && !data_digests) return fail(CEC_EINVAL, "%s: data_digests is NULL and install != 0", op);
    for (int j = 0; install && j < k; ++j)
        if (!data_digests[j]) return fail(CEC_EINVAL, "%s: data_digests[%d] is NULL and install != 0", op, j);
    uint8_t *kept[CEC_MAX_M] = {};  // the digests of the live parities only
    for (int p = 0; p < m; ++p) {
        if (!parity[p]) continue;  // a lost parity: skipped in both launches
        if (!parity_digests || !parity_digests[p])
            return fail(CEC_EINVAL, "%s: parity_digests[%d] is NULL and parity[%d] is written", op, p, p);
        kept[p] = parity_digests[p];
    }
    DigestSet ds;
    if (int r = digest_set_prepare(op, k, m, matrix, data, staging, install ? data_digests : nullptr, kept, n_units,
                                   plan, &ds))
        return r;
    // (cec_diff_update's own checks are all made above: its launch cannot be refused for the
    // arguments, and plans no more tiles than the digest launch just planned)
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int r = digest_set_launch(ds, s)) return r;
    const uint64_t seq = t_last_launch.seq;
    const int rc = cec_diff_update(k, m, matrix, data, staging, parity, install, plan, stream);
    if (rc == CEC_OK) return rc;
    char why[256];
    snprintf(why, sizeof why, "%s", g_err);
    if (t_last_launch.seq != seq)
        return fail(rc, "%s: cec_diff_update failed after %llu of its launches (%s); arenas and digests of the plan's "
                        "units are uncertain: re-base the digests with cec_digest_region", op,
                    static_cast<unsigned long long>(t_last_launch.seq - seq), why);
    // no arena byte changed, and staging is as it was: the same launch again restores the digests
    if (digest_set_launch(ds, s) != CEC_OK)
        return fail(rc, "%s: cec_diff_update failed (%s) and so did the launch that restores the digests; the digests "
                        "of the plan's units are uncertain: re-base them with cec_digest_region of arena + 4096 * u "
                        "into digests + 32 * u", op, why);
    return fail(rc, "%s: cec_diff_update failed (%s); arenas and digests are as before the call", op, why);
}

// One launch: the digests of parities [p0, p0 + lt) against the k data digests, one lane
// per unit.  Reads no arena and no tile: the source only counts the units.
static int digest_check_launch(int dev, cec_scrub_report *s, int k, int m, const int *matrix,
                               const uint8_t *const *data, const uint8_t *const *parity, int p0, int lt,
                               const TileSource &src, hipStream_t stream) {
    const std::vector<Pattern> pats = scrub_patterns(Code{k, m, matrix}, p0, lt);
    DigestCheckArgs a;
    memset(&a, 0, sizeof a);
    for (int i = 0; i < k + lt; ++i) a.dig[i] = i < k ? data[i] : parity[p0 + i - k];
    a.words = s->d_buf + kScrubHead;
    a.counter = s->d_buf;
    a.n_units = static_cast<uint32_t>(src.n_tiles);  // (<= the report's max_tiles <= kScrubMaxTiles)
    a.syn_shift = static_cast<uint32_t>(p0);
    Launch l;
    l.plan = plan_digest_check(k, lt, src.n_tiles);
    l.tb = Tables{nullptr, pats.size(), pats.data(), nullptr};
    l.bases = a.dig;
    l.en = k;
    l.el = lt;
    l.uses[0] = &s->uses;
    return enqueue_launch(dev, stream, l, [&](const LaunchPlan &lp, const uint8_t *d) {
        a.pattern = reinterpret_cast<const Pattern *>(d);
        launch_digest_check(a, lp, stream);
        return CEC_OK;
    });
}

CEC_API int cec_scrub_digests(cec_scrub_report *s, int k, int m, const int *matrix,
                              const uint8_t *const *data_digests, const uint8_t *const *parity_digests,
                              const cec_plan *plan, void *stream) {
    if (!plan) return fail(CEC_EINVAL, "cec_scrub_digests: plan is NULL");
    if (int r = single_pattern_plan(plan, "cec_scrub_digests")) return r;
    return scrub_common("cec_scrub_digests", true, s, k, m, matrix, data_digests, parity_digests, plan, 0, stream);
}

CEC_API int cec_scrub_digests_region(cec_scrub_report *s, int k, int m, const int *matrix,
                                     const uint8_t *const *data_digests, const uint8_t *const *parity_digests,
                                     size_t len, void *stream) {
    return scrub_common("cec_scrub_digests_region", true, s, k, m, matrix, data_digests, parity_digests, nullptr, len,
                        stream);
}

// A process's check of itself: the digest check of the code k = 1, m = 1, matrix {1, 1}, with
// `fresh` as the data digests and `live` as the parity's -- the syndrome is live ^ fresh.
CEC_API int cec_digest_verify_region(cec_scrub_report *s, const uint8_t *live, const uint8_t *fresh, size_t len,
                                     void *stream) {
    static const int kSelf[2] = {1, 1};
    if (!live || !fresh) return fail(CEC_EINVAL, "cec_digest_verify_region: NULL digest array");
    return scrub_common("cec_digest_verify_region", true, s, 1, 1, kSelf, &fresh, &live, nullptr, len, stream);
}
