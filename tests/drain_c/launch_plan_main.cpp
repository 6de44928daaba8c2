// The launch decisions of cec_launchplan.hpp against their documented rules, each rule
// restated here in its own words (never taken from the header): which kernel a shape takes,
// the capacity rung, the grid and the limits of one dispatch, the workgroup split, the store
// policy and its tail, the occupancy cap, the argument-block check, the tiles of an extent.
// Includes the shipped header; built with ASan + UBSan by tests/test_abi.py.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "cec_launchplan.hpp"

using namespace cec;

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            exit(1);                                                  \
        }                                                             \
    } while (0)

static const uint64_t kU32 = 0xFFFFFFFFull;
static const size_t kLdsPerCu = 160 * 1024;
static const uintptr_t kAligned = 0x7f0000001000ull;

static Knobs knobs(int forced_split = -1) {
    Knobs k;  // the defaults: auto policy, 512 MiB, a 96 MiB tail, four waves per digest workgroup
    k.forced_split = forced_split;
    return k;
}

static int ceil_rung(int v, std::initializer_list<int> rungs) {
    for (int r : rungs)
        if (v <= r) return r;
    CHECK(false);
    return 0;
}

// acc classes: 0 none, 1 all, 2 all but the last, 3 anything else (the first output writes,
// the others accumulate)
static Pattern shape_pattern(int n_in, int n_out, int acc_class, int top_slot) {
    Pattern p = {};
    p.n_in = n_in;
    p.n_out = n_out;
    for (int i = 0; i < n_in; ++i) p.in_stream[i] = 0;
    for (int l = 0; l < n_out; ++l) {
        p.out_stream[l] = 1;
        p.out_mode[l] = acc_class == 0 ? kModeWrite
                        : acc_class == 1 ? kModeXor
                        : acc_class == 2 ? (l == n_out - 1 ? kModeWrite : kModeXor)
                                         : (l == 0 ? kModeWrite : kModeXor);
    }
    p.out_stream[n_out - 1] = top_slot;
    return p;
}

static bool listed_exact(int n, int l, int acc) {  // the 40 shapes
    if (acc == CEC_ACC_NONE) return n >= 1 && n <= 8 && l >= 1 && l <= 4;
    if (acc == CEC_ACC_ALL) return (n == 1 && l == 1) || (n == 2 && l >= 1 && l <= 4);
    if (acc == CEC_ACC_ALL_BUT_LAST) return n == 2 && l >= 2 && l <= 4;
    return false;
}

typedef std::tuple<int, int, int, int, bool> Inst;  // kind, nt, lt, acc, released

static void check_kind_and_capacity() {
    std::set<Inst> seen[2], want;
    int n_listed = 0;
    for (int n = 1; n <= 16; ++n)
        for (int l = 1; l <= 4; ++l)
            for (int acc : {CEC_ACC_NONE, CEC_ACC_ALL, CEC_ACC_ALL_BUT_LAST}) n_listed += listed_exact(n, l, acc);
    CHECK(n_listed == 40);
    for (int n = 1; n <= 16; ++n)
        for (int l = 1; l <= 4; ++l)
            for (int cls = 0; cls < 4; ++cls)
                for (int top : {1, 2, kMaxStreams - 1})
                    for (int lds = 0; lds < 2; ++lds)
                        for (uint32_t flags : {0u, kFlagSysRelease}) {
                            if (l == 1 && cls >= 2) continue;  // (one output: none or all)
                            const std::vector<Pattern> pats(1, shape_pattern(n, l, cls, top));
                            const LaunchShape sh = launch_shape(pats, nullptr);
                            CHECK(sh.nt == n && sh.lt == l && sh.streams == top + 1);
                            const LaunchPlan p = plan_combine(sh, 5, 5, kAligned, lds, flags, knobs(), 0, kLdsPerCu);
                            CHECK(p.refusal == kPlanOk);
                            const int acc = cls;  // (the classes are numbered as CEC_ACC_*)
                            if (listed_exact(n, l, acc)) {
                                const bool narrow = n == 1 && l == 1 && top <= 1;
                                CHECK(p.kind == (narrow ? CEC_KERNEL_NARROW : CEC_KERNEL_EXACT));
                                CHECK(p.nt == n && p.lt == l && p.acc == acc);
                            } else {
                                CHECK(p.kind == CEC_KERNEL_GENERIC && p.acc == CEC_ACC_RUNTIME);
                                CHECK(p.nt == ceil_rung(n, {2, 4, 8, 16}) && p.lt == ceil_rung(l, {1, 2, 4}));
                            }
                            CHECK(p.engine == (lds ? CEC_ENGINE_LDS : CEC_ENGINE_PERM));
                            CHECK((p.flags & kFlagSysRelease) == flags && p.n_tiles == 5);
                            seen[lds].insert(Inst(p.kind, p.nt, p.lt, p.acc,
                                                  p.kind == CEC_KERNEL_NARROW && (p.flags & kFlagSysRelease)));
                            // with a pattern of another shape beside it no exact kernel serves:
                            // the rung that holds the larger of each count
                            const int other = n == 1 ? 2 : 1;
                            const std::vector<Pattern> mixed = {pats[0], shape_pattern(other, 1, 0, 1)};
                            const LaunchPlan g = plan_combine(launch_shape(mixed, nullptr), 5, 5, kAligned, lds, flags,
                                                              knobs(), 0, kLdsPerCu);
                            CHECK(g.refusal == kPlanOk && g.kind == CEC_KERNEL_GENERIC && g.acc == CEC_ACC_RUNTIME);
                            CHECK(g.nt == ceil_rung(std::max(n, other), {2, 4, 8, 16}) && g.lt == ceil_rung(l, {1, 2, 4}));
                            seen[lds].insert(Inst(g.kind, g.nt, g.lt, g.acc, false));
                        }
    // what the library compiles per engine: 4 narrow + 40 exact + 12 capacity kernels
    for (int acc : {CEC_ACC_NONE, CEC_ACC_ALL})
        for (bool rel : {false, true}) want.insert(Inst(CEC_KERNEL_NARROW, 1, 1, acc, rel));
    for (int n = 1; n <= 8; ++n)
        for (int l = 1; l <= 4; ++l) want.insert(Inst(CEC_KERNEL_EXACT, n, l, CEC_ACC_NONE, false));
    want.insert(Inst(CEC_KERNEL_EXACT, 1, 1, CEC_ACC_ALL, false));
    for (int l = 1; l <= 4; ++l) want.insert(Inst(CEC_KERNEL_EXACT, 2, l, CEC_ACC_ALL, false));
    for (int l = 2; l <= 4; ++l) want.insert(Inst(CEC_KERNEL_EXACT, 2, l, CEC_ACC_ALL_BUT_LAST, false));
    for (int nt : {2, 4, 8, 16})
        for (int lt : {1, 2, 4}) want.insert(Inst(CEC_KERNEL_GENERIC, nt, lt, CEC_ACC_RUNTIME, false));
    CHECK(want.size() == 4 + 40 + 12 && seen[0] == want && seen[1] == want);

    // patterns of two shapes: no exact kernel, the capacities are the largest of each;
    // a pattern no tile names does not count
    std::vector<Pattern> two = {shape_pattern(3, 2, 0, 1), shape_pattern(5, 1, 0, 1)};
    const std::vector<char> both = {1, 1}, first = {1, 0};
    LaunchPlan p = plan_combine(launch_shape(two, &both), 5, 5, kAligned, false, 0, knobs(), 0, kLdsPerCu);
    CHECK(p.kind == CEC_KERNEL_GENERIC && p.nt == 8 && p.lt == 2 && p.acc == CEC_ACC_RUNTIME);
    p = plan_combine(launch_shape(two, &first), 5, 5, kAligned, false, 0, knobs(), 0, kLdsPerCu);
    CHECK(p.kind == CEC_KERNEL_EXACT && p.nt == 3 && p.lt == 2 && p.acc == CEC_ACC_NONE);
    // nothing to launch: no tile, no pattern used, no output; a shape past the ladder is refused
    CHECK(plan_combine(launch_shape(two, &both), 0, 0, kAligned, false, 0, knobs(), 0, kLdsPerCu).refusal == kPlanNothing);
    const std::vector<char> none = {0, 0};
    CHECK(plan_combine(launch_shape(two, &none), 5, 5, kAligned, false, 0, knobs(), 0, kLdsPerCu).refusal == kPlanNothing);
    LaunchShape big;
    big.nt = 17;
    big.lt = 1;
    CHECK(plan_combine(big, 5, 5, kAligned, false, 0, knobs(), 0, kLdsPerCu).refusal == kPlanNoKernel);

    // the scrub and the digest check: the ladder from 4; the scrub's three exact codes
    std::set<std::tuple<int, int, bool>> scrub, check;
    for (int k = 1; k <= 16; ++k)
        for (int lt = 1; lt <= 4; ++lt)
            for (int whole = 0; whole < 2; ++whole) {
                const bool exact = whole && ((k == 3 && lt == 2) || (k == 4 && lt == 2) || (k == 6 && lt == 3));
                const int nt = exact ? k : ceil_rung(k, {4, 8, 16}), l = exact ? lt : ceil_rung(lt, {1, 2, 4});
                const LaunchPlan s = plan_scrub(k, lt, whole, 7, 7, kAligned, knobs(), 0, kLdsPerCu);
                CHECK(s.refusal == kPlanOk && s.kind == CEC_KERNEL_SCRUB && s.nt == nt && s.lt == l);
                CHECK(s.acc == CEC_ACC_ALL && s.engine == CEC_ENGINE_PERM && s.flags == 0 && s.wt_from == kNoWtTail);
                CHECK(scrub_exact(k, lt, whole) == exact);
                scrub.insert(std::make_tuple(s.nt, s.lt, exact));
                const LaunchPlan c = plan_digest_check(k, lt, 7);
                CHECK(c.refusal == kPlanOk && c.kind == CEC_KERNEL_DIGEST_CHECK && c.acc == CEC_ACC_ALL);
                CHECK(c.nt == ceil_rung(k, {4, 8, 16}) && c.lt == ceil_rung(lt, {1, 2, 4}));
                CHECK(c.split_shift == 0 && c.flags == 0 && c.lds_bytes == 0 && c.block == 256 && c.grid == 1);
                check.insert(std::make_tuple(c.nt, c.lt, false));
            }
    CHECK(scrub.size() == 3 + 9 && check.size() == 9);
}

static void check_grid_and_limits() {
    const std::vector<Pattern> pats(1, shape_pattern(3, 2, 0, 1));
    const LaunchShape sh = launch_shape(pats, nullptr);
    for (uint64_t n : {uint64_t(1), (uint64_t(1) << 30) - 1, uint64_t(1) << 30, kU32})
        for (int s = 0; s <= 2; ++s) {
            const LaunchPlan p = plan_combine(sh, n, n, kAligned, false, 0, knobs(s), 0, kLdsPerCu);
            const uint64_t block = 256u >> s;
            CHECK(p.refusal == kPlanOk && p.split_shift == uint32_t(s) && p.block == block && p.n_tiles == n);
            CHECK(p.grid == std::min<uint64_t>(n << s, kU32 / block));
            CHECK(uint64_t(p.grid) * p.block <= kU32 && p.grid >= 1);
        }
    CHECK(plan_combine(sh, kU32 + 1, 0, kAligned, false, 0, knobs(), 0, kLdsPerCu).refusal == kPlanTooLarge);

    // the scrub and the digest check: one workgroup per part of a tile, one lane per unit
    const uint64_t scrub_max = kU32 / 256;
    CHECK(kScrubMaxTiles == scrub_max);
    for (int s = 0; s <= 2; ++s)
        for (uint64_t n : {scrub_max - 1, scrub_max}) {
            const LaunchPlan p = plan_scrub(3, 2, true, n, n, kAligned, knobs(s), 0, kLdsPerCu);
            CHECK(p.refusal == kPlanOk && p.grid == n << s && p.block == 256u >> s && p.split_shift == uint32_t(s));
            CHECK(uint64_t(p.grid) * p.block <= kU32);
            const LaunchPlan c = plan_digest_check(3, 2, n);
            CHECK(c.refusal == kPlanOk && c.grid == (n + 255) / 256 && uint64_t(c.grid) * c.block >= n);
        }
    CHECK(plan_scrub(3, 2, true, scrub_max + 1, 0, kAligned, knobs(), 0, kLdsPerCu).refusal == kPlanTooLarge);
    CHECK(plan_scrub(3, 2, true, 0, 0, kAligned, knobs(), 0, kLdsPerCu).refusal == kPlanNothing);
    CHECK(plan_digest_check(3, 2, scrub_max + 1).refusal == kPlanTooLarge);
    CHECK(plan_digest_check(3, 2, 0).refusal == kPlanNothing);

    // the digests: one wave per (tile, arena) or per tile, 2^32 - 1 lanes in one dispatch
    const uint64_t work_max = kU32 / 256 * 4;
    CHECK(kDigestMaxWork == work_max);
    for (int ws = 0; ws <= 2; ++ws)
        for (int n : {1, 3, 24})
            for (uint64_t tiles : {work_max / n - 1, work_max / n}) {
                Knobs kn = knobs();
                kn.digest_waves_shift = ws;
                const LaunchPlan p = plan_digest(n, tiles, kn);
                const uint64_t per_wg = uint64_t(1) << ws;
                CHECK(p.refusal == kPlanOk && p.kind == CEC_KERNEL_DIGEST && p.nt == n && p.lt == 0);
                CHECK(p.block == 64 * per_wg && p.grid == (tiles * n + per_wg - 1) / per_wg);
                CHECK(uint64_t(p.grid) * p.block <= kU32 && p.acc == CEC_ACC_NONE && p.n_tiles == tiles);
                CHECK(plan_digest(n, work_max / n + 1, kn).refusal == kPlanTooLarge);
            }
    CHECK(plan_digest(3, 0, knobs()).refusal == kPlanNothing);
    for (uint64_t tiles : {uint64_t(1), uint64_t(4), uint64_t(5), work_max - 1, work_max}) {
        const LaunchPlan p = plan_digest_update(tiles);
        CHECK(p.refusal == kPlanOk && p.kind == CEC_KERNEL_DIGEST_UPDATE && p.nt == 1 && p.lt == 0);
        CHECK(p.grid == (tiles + 3) / 4 && p.block == 256 && uint64_t(p.grid) * p.block <= kU32);
        CHECK(p.acc == CEC_ACC_ALL);
    }
    CHECK(plan_digest_update(work_max + 1).refusal == kPlanTooLarge);
}

static void check_split() {
    // four one-wave workgroups per tile when at least 3/4 of the tiles are full line tiles
    // and no base has a bit below 128 set; else one workgroup
    CHECK(split_shift_for(knobs(), kAligned, 8, 6) == 2);
    CHECK(split_shift_for(knobs(), kAligned, 8, 5) == 0);
    CHECK(split_shift_for(knobs(), kAligned, 4, 3) == 2 && split_shift_for(knobs(), kAligned, 4, 2) == 0);
    for (uintptr_t bit = 1; bit < 128; bit <<= 1) CHECK(split_shift_for(knobs(), kAligned | bit, 8, 8) == 0);
    CHECK(split_shift_for(knobs(), kAligned | 128, 8, 8) == 2);
    for (int f = 0; f <= 2; ++f) {
        CHECK(split_shift_for(knobs(f), kAligned | 1, 8, 0) == uint32_t(f));
        CHECK(split_shift_for(knobs(f), kAligned, 8, 8) == uint32_t(f));
    }
}

static void check_store() {
    Knobs kn = knobs();
    kn.wt_max_bytes = 1 << 20;
    kn.wt_tail_bytes = 10 << 10;
    // up to wt_max streamed bytes: the whole launch writes through
    StoreChoice c = write_through(kn, 100, 0, 2, 1 << 20);
    CHECK(c.all && c.from == kNoWtTail);
    // past it: the last ceil(tail / (lt * (4096 >> s))) work items
    for (int s = 0; s <= 2; ++s)
        for (int lt = 1; lt <= 4; ++lt) {
            const uint64_t per_item = uint64_t(lt) * (4096 >> s), items = ((10 << 10) + per_item - 1) / per_item;
            c = write_through(kn, 100, s, lt, (1 << 20) + 1);
            CHECK(!c.all && c.from == (uint64_t(100) << s) - items);
        }
    // a tail of the whole launch or more is a write-through launch
    kn.wt_tail_bytes = 2 * 100 * 4096;
    c = write_through(kn, 100, 1, 2, (1 << 20) + 1);
    CHECK(c.all && c.from == kNoWtTail);
    kn.wt_tail_bytes = 2 * 100 * 4096 - 1;  // (still every work item: the count rounds up)
    CHECK(write_through(kn, 100, 1, 2, (1 << 20) + 1).all);
    kn.wt_tail_bytes = 2 * 100 * 4096 - 4096;
    c = write_through(kn, 100, 1, 2, (1 << 20) + 1);
    CHECK(!c.all && c.from == 1);
    // no tail: tail 0, no output, a forced policy
    kn.wt_tail_bytes = 0;
    c = write_through(kn, 100, 0, 2, (1 << 20) + 1);
    CHECK(!c.all && c.from == kNoWtTail);
    kn.wt_tail_bytes = 10 << 10;
    c = write_through(kn, 100, 0, 0, (1 << 20) + 1);
    CHECK(!c.all && c.from == kNoWtTail);
    for (int policy : {int(kStoreNt), int(kStoreWt)})
        for (uint64_t streamed : {uint64_t(1), uint64_t(1) << 40}) {
            kn.store_policy = policy;
            c = write_through(kn, 100, 0, 2, streamed);
            CHECK(c.all == (policy == kStoreWt) && c.from == kNoWtTail);
        }
    // in a plan: streamed = tiles * 4096 * (inputs + outputs); only the PERM engine's full
    // kernels carry a tail, the narrow and the LDS engine's never
    kn = knobs(0);
    kn.wt_max_bytes = 100 * 4096 * 5;
    kn.wt_tail_bytes = 10 << 10;
    const std::vector<Pattern> enc(1, shape_pattern(3, 2, 0, 4)), mul(1, shape_pattern(1, 1, 1, 1));
    LaunchPlan p = plan_combine(launch_shape(enc, nullptr), 100, 100, kAligned, false, 0, kn, 0, kLdsPerCu);
    CHECK(p.flags == kFlagWriteThrough && p.wt_from == kNoWtTail);
    p = plan_combine(launch_shape(enc, nullptr), 101, 101, kAligned, false, 0, kn, 0, kLdsPerCu);
    CHECK(p.flags == kFlagWtTail && p.wt_from == 101 - 2);  // 10 KiB of 2 x 4 KiB per tile: 2 tiles
    p = plan_combine(launch_shape(enc, nullptr), 101, 101, kAligned, true, 0, kn, 0, kLdsPerCu);
    CHECK(p.flags == 0 && p.wt_from == kNoWtTail);
    kn.wt_max_bytes = 0;
    p = plan_combine(launch_shape(mul, nullptr), 101, 101, kAligned, false, kFlagSysRelease, kn, 0, kLdsPerCu);
    CHECK(p.kind == CEC_KERNEL_NARROW && p.flags == kFlagSysRelease && p.wt_from == kNoWtTail);
}

static void check_occupancy() {
    for (int s = 0; s <= 2; ++s) {
        CHECK(occupancy_lds(0, kLdsPerCu, s) == 0 && occupancy_lds(-3, kLdsPerCu, s) == 0);
        size_t prev = 65536;
        for (int cap = 1; cap <= 64; ++cap) {
            // LDS per workgroup so that only cap / (waves per workgroup) workgroups fit a CU,
            // 256 B below the boundary, at most what one workgroup may ask for
            const int wgs = std::max(1, cap / std::max(1, (256 >> s) / 64));
            const size_t lds = occupancy_lds(cap, kLdsPerCu, s);
            CHECK(lds == std::min<size_t>(65536, kLdsPerCu / wgs - 256));
            CHECK(lds <= 65536 && lds <= prev && size_t(wgs + 1) * lds > kLdsPerCu - 65536);
            prev = lds;
        }
    }
    // in a plan: the larger of the LDS engine's rows and the cap
    std::vector<Pattern> enc(1, shape_pattern(3, 2, 0, 4));
    enc[0].lds_rows = 5;
    CHECK(plan_combine(launch_shape(enc, nullptr), 9, 9, kAligned, true, 0, knobs(), 0, kLdsPerCu).lds_bytes == 5 * 256);
    CHECK(plan_combine(launch_shape(enc, nullptr), 9, 9, kAligned, false, 0, knobs(), 0, kLdsPerCu).lds_bytes == 0);
    CHECK(plan_combine(launch_shape(enc, nullptr), 9, 9, kAligned, true, 0, knobs(0), 32, kLdsPerCu).lds_bytes ==
          kLdsPerCu / 8 - 256);
    CHECK(plan_scrub(3, 2, true, 9, 9, kAligned, knobs(2), 32, kLdsPerCu).lds_bytes == kLdsPerCu / 32 - 256);
}

static void check_layout_rule() {
    const uint8_t *full[kMaxStreams];
    for (int i = 0; i < kMaxStreams; ++i) full[i] = reinterpret_cast<const uint8_t *>(kAligned + 4096 * i);
    for (int narrow = 0; narrow < 2; ++narrow) {
        const int slots = narrow ? kNarrowStreams : kMaxStreams, n_in = narrow ? 1 : 3, n_out = narrow ? 1 : 2;
        Pattern good = {};
        good.n_in = n_in;
        good.n_out = n_out;
        for (int i = 0; i < n_in; ++i) good.in_stream[i] = narrow ? 0 : slots - 1 - i;
        for (int l = 0; l < n_out; ++l) good.out_stream[l] = narrow ? 1 : l;
        LaunchPlan lp;
        lp.kind = narrow ? CEC_KERNEL_NARROW : CEC_KERNEL_EXACT;
        CHECK(stream_layout_ok(full, slots, Tables{nullptr, 1, &good, nullptr}));
        check_layout(lp, full, Tables{nullptr, 1, &good, nullptr});
        CHECK(lp.refusal == kPlanOk);
        for (int pos = 0; pos < n_in + n_out; ++pos) {
            int32_t &slot = pos < n_in ? good.in_stream[pos] : good.out_stream[pos - n_in];
            const int32_t kept = slot;
            for (int32_t past : {slots, slots + 1, int32_t(kMaxStreams), int32_t(1000)}) {  // a slot the block lacks
                slot = past;
                CHECK(!stream_layout_ok(full, slots, Tables{nullptr, 1, &good, nullptr}));
                LaunchPlan bad = lp;
                check_layout(bad, full, Tables{nullptr, 1, &good, nullptr});
                CHECK(bad.refusal == kPlanLayout);
            }
            slot = kept;
            const uint8_t *holed[kMaxStreams];  // an empty base
            for (int i = 0; i < kMaxStreams; ++i) holed[i] = i == kept ? nullptr : full[i];
            CHECK(!stream_layout_ok(holed, slots, Tables{nullptr, 1, &good, nullptr}));
            CHECK(stream_layout_ok(full, slots, Tables{nullptr, 1, &good, nullptr}));
        }
        // patterns no tile names are ignored, whatever they hold; one that is named is not
        Pattern two[2] = {good, good};
        two[1].in_stream[0] = slots;
        const std::vector<char> first = {1, 0}, both = {1, 1}, shorter = {1};
        CHECK(stream_layout_ok(full, slots, Tables{nullptr, 2, two, &first}));
        CHECK(stream_layout_ok(full, slots, Tables{nullptr, 2, two, &shorter}));
        CHECK(!stream_layout_ok(full, slots, Tables{nullptr, 2, two, &both}));
        CHECK(!stream_layout_ok(full, slots, Tables{nullptr, 2, two, nullptr}));
    }
    // the scrub's and the digest check's blocks have 24 slots
    Pattern sp = {};
    sp.n_in = 16;
    sp.n_out = 4;
    for (int i = 0; i < 16; ++i) sp.in_stream[i] = i;
    for (int l = 0; l < 4; ++l) sp.out_stream[l] = 16 + l;
    for (int kind : {CEC_KERNEL_SCRUB, CEC_KERNEL_DIGEST_CHECK}) {
        LaunchPlan lp;
        lp.kind = kind;
        check_layout(lp, full, Tables{nullptr, 1, &sp, nullptr});
        CHECK(lp.refusal == kPlanOk);
        sp.out_stream[3] = 24;
        check_layout(lp, full, Tables{nullptr, 1, &sp, nullptr});
        CHECK(lp.refusal == kPlanLayout);
        sp.out_stream[3] = 19;
    }
}

static void check_tiles() {
    const uint64_t bases[] = {0, uint64_t(1) << 40};
    const uint64_t around[] = {0, 1, 16, 127, 128, 129, 4095, 4096, 4097, 4224, 8191, 8192};
    for (uint64_t base : bases)
        for (uint64_t rel : around)
            for (uint32_t len : {1u, 4095u, 4096u, 4097u, 8193u}) {
                const uint64_t off = base + rel, src = 777 + rel;
                std::vector<Tile> t(tiles_of(off, len));  // (exactly: ASan sees one tile too many)
                CHECK(append_tiles(t.data(), off, src, len, 9) == t.size());
                CHECK(t.size() == (off + len - 1) / 4096 - off / 4096 + 1);
                uint64_t at = off;
                int64_t lines = 0;
                for (const Tile &x : t) {
                    CHECK(x.off == at && x.src_off == src + (at - off) && x.pattern == 9);
                    CHECK(x.len >= 1 && x.len <= 4096 && x.off / 4096 == (x.off + x.len - 1) / 4096);
                    lines += x.len == 4096 && x.off % 128 == 0;
                    at += x.len;
                }
                CHECK(at == off + len && count_line_tiles(t.data(), t.size()) == lines);
            }
    CHECK(tiles_of(5, 0) == 0 && append_tiles(nullptr, 5, 5, 0, 0) == 0 && count_line_tiles(nullptr, 0) == 0);
}

static void check_knobs_from_env() {
    for (const char *name : {"CEC_SPLIT_SHIFT", "CEC_STORE_POLICY", "CEC_WT_MAX_BYTES", "CEC_WT_TAIL_BYTES",
                             "CEC_DIGEST_WAVES_SHIFT"})
        unsetenv(name);
    Knobs k = Knobs::from_env();
    CHECK(k.forced_split == -1 && k.store_policy == kStoreAuto && k.wt_max_bytes == uint64_t(512) << 20);
    CHECK(k.wt_tail_bytes == uint64_t(96) << 20 && k.digest_waves_shift == 2);
    setenv("CEC_SPLIT_SHIFT", "7", 1);
    setenv("CEC_STORE_POLICY", "wt", 1);
    setenv("CEC_WT_MAX_BYTES", "0x1000", 1);
    setenv("CEC_WT_TAIL_BYTES", "0", 1);
    setenv("CEC_DIGEST_WAVES_SHIFT", "1", 1);
    k = Knobs::from_env();
    CHECK(k.forced_split == 2 && k.store_policy == kStoreWt && k.wt_max_bytes == 4096 && k.wt_tail_bytes == 0);
    CHECK(k.digest_waves_shift == 1);
    setenv("CEC_STORE_POLICY", "WT", 1);   // (each of the three is reported on stderr)
    setenv("CEC_WT_MAX_BYTES", "-1", 1);
    setenv("CEC_WT_TAIL_BYTES", " 4096", 1);
    k = Knobs::from_env();
    CHECK(k.store_policy == kStoreAuto && k.wt_max_bytes == uint64_t(512) << 20 && k.wt_tail_bytes == uint64_t(96) << 20);
}

int main() {
    check_kind_and_capacity();
    check_grid_and_limits();
    check_split();
    check_store();
    check_occupancy();
    check_layout_rule();
    check_tiles();
    check_knobs_from_env();
    printf("ok\n");
    return 0;
}
