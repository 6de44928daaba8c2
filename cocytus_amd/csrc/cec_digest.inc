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
// The bulk paths keep them in the launch that moves the bytes: cec_encode_digests,
// cec_encode_region_digests and cec_decode_digests run the encode's and the decode's
// combinations (encode_combo, decode_combos) through run_combos_digests, whose kernel emits
// the digest of every unit it reads and writes.
// Built from the library's parts: a TileSource to walk, the planners of cec_launchplan.hpp
// (plan_digest, plan_digest_update, plan_digest_set, plan_combine_digest, plan_digest_check),
// scrub_patterns for the check's coefficients, enqueue_launch.

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

// ---- digest-emitting combinations: cec_encode_digests, cec_decode_digests ----
static_assert(CEC_KERNEL_COMBINE_DIGEST == 8, "cec_launch_record::kind");

// The live digest arrays of a launch's streams: dig[slot] goes with Streams::base[slot]
// (NULL: that stream's digests are not kept).
struct DigestSlots {
    uint8_t *dig[kMaxStreams] = {};
};

// The plan's output capacity: combine_digest_kernel<1>, <2> or <4> (three instantiations).
static void launch_combine_digest(const CombineDigestArgs &a, const LaunchPlan &lp, hipStream_t s) {
    if (lp.lt == 1) hipLaunchKernelGGL(combine_digest_kernel<1>, dim3(lp.grid), dim3(lp.block), 0, s, a);
    else if (lp.lt == 2) hipLaunchKernelGGL(combine_digest_kernel<2>, dim3(lp.grid), dim3(lp.block), 0, s, a);
    else hipLaunchKernelGGL(combine_digest_kernel<4>, dim3(lp.grid), dim3(lp.block), 0, s, a);
}

// run_combos for the digest-emitting kernel, for any list of combinations whose outputs are
// all written (kModeWrite): one launch per kPatL outputs, as build_patterns splits them, each
// writing its outputs' bytes and their digests together; the inputs' digests go with the first
// launch only.  Every tile of `src` must obey the unit rule (the caller checks it: it knows
// the arena length).  Everything is checked, built and planned before the first launch, so a
// refusal launches nothing; always the PERM engine.
static int run_combos_digests(const char *op, int dev, const Streams &st, const DigestSlots &dg,
                              const std::vector<Combo> &combos, const TileSource &src, hipStream_t stream) {
    t_last_engine = CEC_ENGINE_PERM;  // whatever cec_set_engine says
    size_t max_out = 0;
    int max_in = 0;
    bool in_digests = false;
    for (const Combo &c : combos) {
        max_out = std::max(max_out, c.outs.size());
        max_in = std::max(max_in, c.n_in);
        for (const Combo::Out &o : c.outs)
            if (o.mode != kModeWrite)
                return fail(CEC_EINVAL, "internal: %s: a read-modify-write output in a digest-emitting launch; "
                                        "not launched", op);
        for (int i = 0; i < std::min(c.n_in, static_cast<int>(kPatN)); ++i) in_digests |= dg.dig[c.in_stream[i]] != nullptr;
    }
    // (a launch of its own for the inputs' digests where nothing is produced: every parity lost)
    const size_t groups = std::max<size_t>((max_out + kPatL - 1) / kPatL, in_digests ? 1 : 0);
    if (src.n_tiles == 0 || groups == 0) return CEC_OK;  // (before the fail hook counts)
    struct Group {
        std::vector<Pattern> pats;
        LaunchPlan plan;
        DigestSlots dig;
        bool in_digests = false;
    };
    std::vector<Group> gs(groups);
    for (size_t g = 0; g < groups; ++g) {
        Group &G = gs[g];
        std::vector<uint8_t> rows;  // (PERM: none)
        if (int r = build_patterns(combos, g, CEC_ENGINE_PERM, G.pats, rows)) return r;
        int lt = 0;
        for (size_t q = 0; q < combos.size(); ++q) {
            const Pattern &p = G.pats[q];
            lt = std::max(lt, p.n_out);
            for (int l = 0; l < p.n_out; ++l) G.dig.dig[p.out_stream[l]] = dg.dig[p.out_stream[l]];
            for (int i = 0; g == 0 && i < p.n_in; ++i) G.dig.dig[p.in_stream[i]] = dg.dig[p.in_stream[i]];
        }
        G.in_digests = g == 0 && in_digests;
        G.plan = plan_combine_digest(max_in, lt, src.n_tiles);
        if (G.plan.refusal == kPlanTooLarge)
            return fail(CEC_EINVAL, "%s: %llu tiles, one launch holds %llu", op,
                        static_cast<unsigned long long>(src.n_tiles), static_cast<unsigned long long>(kDigestMaxWork));
        if (G.plan.refusal != kPlanOk)
            return fail(CEC_EINVAL, "internal: %s: no digest-emitting kernel for %d x %d; not launched", op, max_in, lt);
    }
    for (Group &G : gs) {
        Launch l;
        l.plan = G.plan;
        if (st.refused) l.plan.refusal = kPlanStreams;
        l.tb = Tables{nullptr, G.pats.size(), G.pats.data(), nullptr};
        l.bases = st.base;
        l.en = G.plan.nt;
        l.el = G.plan.lt;
        l.uses[0] = src.uses;  // a plan's streams, for its destroy
        const int rc = enqueue_launch(dev, stream, l, [&](const LaunchPlan &lp, const uint8_t *d) {
            CombineDigestArgs a;
            memset(&a, 0, sizeof a);
            for (int i = 0; i < kMaxStreams; ++i) {
                a.base[i] = st.base[i];
                a.dig[i] = G.dig.dig[i];
            }
            a.tiles = src.tiles;
            a.implicit_len = src.implicit_len;
            a.patterns = reinterpret_cast<const Pattern *>(d);
            a.n_tiles = static_cast<uint32_t>(lp.n_tiles);  // (<= kDigestMaxWork)
            a.in_digests = G.in_digests;
            launch_combine_digest(a, lp, stream);
            return CEC_OK;
        });
        if (rc) return rc;
    }
    return CEC_OK;
}

// A digest array an op was handed: NULL (not kept) or 16-byte aligned.
static int digest_array_ok(const char *op, const char *what, int i, const uint8_t *d) {
    if (reinterpret_cast<uintptr_t>(d) & 15) return fail(CEC_EINVAL, "%s: %s[%d] is not 16-byte aligned", op, what, i);
    return CEC_OK;
}

// The unit rule (cec_launchplan.hpp) on what an op walks: the plan's tiles, or the region
// [0, len) of an arena of arena_len bytes.
static int unit_rule_ok(const char *op, const cec_plan *plan, uint64_t len, uint64_t arena_len) {
    if (!plan) {
        if (const UnitBreach b = unit_rule_region(len, arena_len))
            return fail(CEC_EINVAL, "%s: the region [0, %llu) %s (arena_len %llu)", op, static_cast<unsigned long long>(len),
                        unit_breach_text(b), static_cast<unsigned long long>(arena_len));
        return CEC_OK;
    }
    size_t bad = 0;
    if (const UnitBreach b = unit_rule_tiles(plan->h_tiles.data(), plan->h_tiles.size(), arena_len, &bad))
        return fail(CEC_EINVAL, "%s: the tile at offset %llu, %u bytes, %s (arena_len %llu): every extent must "
                                "be whole 4096-byte units", op, static_cast<unsigned long long>(plan->h_tiles[bad].off),
                    plan->h_tiles[bad].len, unit_breach_text(b), static_cast<unsigned long long>(arena_len));
    return CEC_OK;
}

static int encode_digests_common(const char *op, int k, int m, const int *matrix, const uint8_t *const *data,
                                 uint8_t *const *parity, uint8_t *const *data_digests,
                                 uint8_t *const *parity_digests, uint64_t arena_len, const cec_plan *plan, uint64_t len,
                                 void *stream) {
    if (int r = check_code(k, m, matrix)) return r;
    if (!data || !parity) return fail(CEC_EINVAL, "%s: NULL arena array", op);
    int dev;
    if (int r = current_device(&dev)) return r;
    EncodeCombo e;
    if (int r = encode_combo(op, Code{k, m, matrix}, data, parity, &e)) return r;
    DigestSlots dg;
    for (int j = 0; j < k && data_digests; ++j) {
        if (int r = digest_array_ok(op, "data_digests", j, data_digests[j])) return r;
        dg.dig[e.s_data[j]] = data_digests[j];
    }
    for (int p = 0; p < m && parity_digests; ++p) {
        if (!parity[p]) continue;  // a lost parity: its digest entry is ignored
        if (int r = digest_array_ok(op, "parity_digests", p, parity_digests[p])) return r;
        dg.dig[e.s_parity[p]] = parity_digests[p];
    }
    TileSource src;
    if (int r = plan ? TileSource::of_plan(plan, dev, &src) : TileSource::of_region(len, &src)) return r;
    if (int r = unit_rule_ok(op, plan, len, arena_len)) return r;
    return run_combos_digests(op, dev, e.st, dg, {e.c}, src, static_cast<hipStream_t>(stream));
}

CEC_API int cec_encode_digests(int k, int m, const int *matrix, const uint8_t *const *data, uint8_t *const *parity,
                               uint8_t *const *data_digests, uint8_t *const *parity_digests, uint64_t arena_len,
                               const cec_plan *plan, void *stream) {
    if (!plan) return fail(CEC_EINVAL, "cec_encode_digests: plan is NULL");
    if (int r = single_pattern_plan(plan, "cec_encode_digests")) return r;
    return encode_digests_common("cec_encode_digests", k, m, matrix, data, parity, data_digests, parity_digests,
                                 arena_len, plan, 0, stream);
}

CEC_API int cec_encode_region_digests(int k, int m, const int *matrix, const uint8_t *const *data,
                                      uint8_t *const *parity, uint8_t *const *data_digests,
                                      uint8_t *const *parity_digests, size_t len, void *stream) {
    return encode_digests_common("cec_encode_region_digests", k, m, matrix, data, parity, data_digests,
                                 parity_digests, len, nullptr, len, stream);
}

CEC_API int cec_decode_digests(int k, int m, const int *matrix, const uint32_t *masks, int n_masks,
                               const uint8_t *const *arenas, uint8_t *const *out, uint8_t *const *out_digests,
                               uint64_t arena_len, const cec_plan *plan, void *stream) {
    const char *op = "cec_decode_digests";
    if (int r = check_code(k, m, matrix)) return r;
    if (!masks || n_masks < 1 || !arenas || !out || !plan) return fail(CEC_EINVAL, "%s: bad args", op);
    int dev;
    if (int r = current_device(&dev)) return r;
    if (plan->n_ext && plan->max_pattern >= static_cast<uint32_t>(n_masks))
        return fail(CEC_EINVAL, "%s: an extent names mask %u of %d", op, plan->max_pattern, n_masks);
    DecodeCombos d;
    if (int r = decode_combos(op, Code{k, m, matrix}, masks, n_masks, arenas, out, &d)) return r;
    // strict about the arrays: every lid the op rebuilds has its digests emitted
    DigestSlots dg;
    for (int j = 0; j < k; ++j) {
        if (!(d.lost & (1u << j))) continue;
        if (!out_digests || !out_digests[j])
            return fail(CEC_EINVAL, "%s: out_digests[%d] is NULL and a mask loses lid %d", op, j, j);
        if (int r = digest_array_ok(op, "out_digests", j, out_digests[j])) return r;
        dg.dig[d.s_out[j]] = out_digests[j];
    }
    TileSource src;
    if (int r = TileSource::of_plan(plan, dev, &src)) return r;
    if (int r = unit_rule_ok(op, plan, 0, arena_len)) return r;
    return run_combos_digests(op, dev, d.st, dg, d.combos, src, static_cast<hipStream_t>(stream));
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
