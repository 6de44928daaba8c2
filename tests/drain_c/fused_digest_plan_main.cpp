// plan_combine_digest and the unit rule of cec_launchplan.hpp against their documented rules,
// restated here.  The plan: one wave per whole unit and four waves per workgroup, so grid =
// ceil(tiles / 4) workgroups of 256 lanes; at most 67,108,860 tiles in one dispatch; the launch
// record is kind 8, nt = the launch's inputs, lt = the output capacity 1, 2 or 4, no
// read-modify-write output, PERM, no split, no flags, no dynamic LDS.  The unit rule: every
// tile starts on a 4 KiB arena boundary and is a whole unit, except a shorter last one that
// ends exactly at arena_len; nothing ends beyond arena_len.  Includes the shipped header; built
// with ASan + UBSan by tests/test_fused_digest.py.  Prints "ok".
#include <cstdio>
#include <cstdlib>
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

static void check_record(const LaunchPlan &p, int nt, int lt, uint64_t tiles, uint32_t grid) {
    CHECK(p.refusal == kPlanOk);
    CHECK(p.kind == 8 && p.kind == CEC_KERNEL_COMBINE_DIGEST);
    CHECK(p.nt == nt && p.lt == lt);
    CHECK(p.acc == CEC_ACC_NONE);
    CHECK(p.engine == CEC_ENGINE_PERM);
    CHECK(p.split_shift == 0 && p.flags == 0);
    CHECK(p.lds_bytes == 0);
    CHECK(p.wt_from == CEC_NO_WT_TAIL);
    CHECK(p.block == 256);
    CHECK(p.n_tiles == tiles);
    CHECK(p.grid == grid);
    CHECK(static_cast<uint64_t>(p.grid) * 4 >= tiles && static_cast<uint64_t>(p.grid - 1) * 4 < tiles);
    CHECK(static_cast<uint64_t>(p.grid) * p.block <= 0xFFFFFFFFull);  // one dispatch
}

// The tiles of extents (off, len), as cec_plan_create makes them, and the rule on them.
struct Ext {
    uint64_t off;
    uint32_t len;
};
static UnitBreach rule(std::vector<Ext> ext, uint64_t arena_len, size_t *bad = nullptr) {
    size_t n = 0;
    for (const Ext &e : ext) n += tiles_of(e.off, e.len);
    std::vector<Tile> t(n + 1);
    size_t at = 0;
    for (const Ext &e : ext) at += append_tiles(t.data() + at, e.off, 0, e.len, 0);
    CHECK(at == n);
    return unit_rule_tiles(t.data(), n, arena_len, bad);
}

int main() {
    const uint64_t kMax = 67108860;  // (2^32 - 1) / 256 workgroups of four waves
    CHECK(kDigestMaxWork == kMax);

    // ---- the plan
    const LaunchPlan none = plan_combine_digest(3, 2, 0);
    CHECK(none.refusal == kPlanNothing && none.grid == 0 && none.kind == CEC_KERNEL_COMBINE_DIGEST);
    check_record(plan_combine_digest(3, 2, 1), 3, 2, 1, 1);
    check_record(plan_combine_digest(3, 2, 3), 3, 2, 3, 1);
    check_record(plan_combine_digest(3, 2, 4), 3, 2, 4, 1);
    check_record(plan_combine_digest(3, 2, 5), 3, 2, 5, 2);
    check_record(plan_combine_digest(3, 2, 9), 3, 2, 9, 3);
    check_record(plan_combine_digest(3, 2, 65536), 3, 2, 65536, 16384);
    check_record(plan_combine_digest(3, 2, kMax), 3, 2, kMax, 16777215);
    CHECK(plan_combine_digest(3, 2, kMax + 1).refusal == kPlanTooLarge);
    CHECK(plan_combine_digest(3, 2, kMax + 1).grid == 0);
    CHECK(plan_combine_digest(3, 2, ~uint64_t(0)).refusal == kPlanTooLarge);
    // the output capacity: 1, 2, 4; a launch that only digests its inputs runs capacity 1
    const int want_lt[5] = {1, 1, 2, 4, 4};
    for (int lt = 0; lt <= 4; ++lt)
        for (int n_in : {1, 3, 5, 16}) check_record(plan_combine_digest(n_in, lt, 7), n_in, want_lt[lt], 7, 2);
    CHECK(combine_digest_capacity(0) == 1 && combine_digest_capacity(3) == 4);
    // shapes past a pattern: no kernel
    CHECK(plan_combine_digest(17, 1, 4).refusal == kPlanNoKernel);
    CHECK(plan_combine_digest(3, 5, 4).refusal == kPlanNoKernel);
    CHECK(plan_combine_digest(-1, 1, 4).refusal == kPlanNoKernel);
    // its argument block has every stream slot: the layout check looks at all of them
    {
        Pattern p;
        memset(&p, 0, sizeof p);
        p.n_in = 1;
        p.n_out = 1;
        p.in_stream[0] = kMaxStreams - 1;
        p.out_stream[0] = kScrubStreams;  // (a slot the scrub kernels' block does not have)
        const uint8_t *bases[kMaxStreams] = {};
        uint8_t byte = 0;
        bases[kMaxStreams - 1] = bases[kScrubStreams] = &byte;
        LaunchPlan ok = plan_combine_digest(1, 1, 4);
        check_layout(ok, bases, Tables{nullptr, 1, &p, nullptr});
        CHECK(ok.refusal == kPlanOk);
        bases[kScrubStreams] = nullptr;
        LaunchPlan bad = plan_combine_digest(1, 1, 4);
        check_layout(bad, bases, Tables{nullptr, 1, &p, nullptr});
        CHECK(bad.refusal == kPlanLayout);
    }

    // ---- the unit rule on one tile
    const uint64_t A = 8 * 4096 + 2064;  // an arena whose ninth unit is ragged
    CHECK(unit_rule_tile(0, 4096, A) == kUnitOk);
    CHECK(unit_rule_tile(4096, 4096, A) == kUnitOk);
    CHECK(unit_rule_tile(16, 4080, A) == kUnitOffset);
    CHECK(unit_rule_tile(16, 4096, A) == kUnitOffset);
    CHECK(unit_rule_tile(8 * 4096, 2064, A) == kUnitOk);        // short, ends at arena_len
    CHECK(unit_rule_tile(8 * 4096, 2048, A) == kUnitPartial);   // ... 16 bytes before it
    CHECK(unit_rule_tile(4096, 2064, A) == kUnitPartial);       // short, not the last unit
    CHECK(unit_rule_tile(8 * 4096, 2080, A) == kUnitBeyond);    // 16 bytes beyond
    CHECK(unit_rule_tile(8 * 4096, 4096, A) == kUnitBeyond);
    CHECK(unit_rule_tile(9 * 4096, 1, A) == kUnitBeyond);
    CHECK(unit_rule_tile(~uint64_t(0) - 4095, 4096, A) == kUnitBeyond);  // (no wrap-around)
    CHECK(unit_rule_tile(0, 1, 1) == kUnitOk);
    CHECK(unit_rule_tile(0, 4096, 4096) == kUnitOk);
    CHECK(unit_rule_tile(0, 4095, 4096) == kUnitPartial);

    // ---- on the tiles of extents
    size_t bad = 99;
    CHECK(rule({}, A) == kUnitOk);
    CHECK(rule({{0, 0}}, A) == kUnitOk);  // (an empty extent has no tile)
    CHECK(rule({{0, 4096}}, A) == kUnitOk);
    CHECK(rule({{0, 3 * 4096}, {5 * 4096, 4096}}, A) == kUnitOk);
    CHECK(rule({{4096, 4096}, {16, 4096}}, A, &bad) == kUnitOffset && bad == 1);  // off at 16
    CHECK(rule({{0, static_cast<uint32_t>(A)}}, A) == kUnitOk);                   // the whole arena
    CHECK(rule({{7 * 4096, 4096 + 2064}}, A) == kUnitOk);                         // short last tile at arena_len
    CHECK(rule({{7 * 4096, 4096 + 2048}}, A, &bad) == kUnitPartial && bad == 1);  // ... 16 bytes before it
    CHECK(rule({{0, 4096}, {2 * 4096, 100}}, A, &bad) == kUnitPartial && bad == 1);
    CHECK(rule({{7 * 4096, 2 * 4096}}, A, &bad) == kUnitBeyond && bad == 1);       // ends beyond arena_len
    CHECK(rule({{0, 4096}, {16 * 4096, 4096}}, A, &bad) == kUnitBeyond && bad == 1);

    // ---- on a region [0, len), which is the whole arena for cec_encode_region_digests
    for (uint64_t len : {uint64_t(0), uint64_t(1), uint64_t(4095), uint64_t(4096), uint64_t(4097)}) {
        CHECK(unit_rule_region(len, len) == kUnitOk);
        // ... and its implicit tiles obey the rule one by one
        for (uint64_t o = 0; o < len; o += 4096)
            CHECK(unit_rule_tile(o, static_cast<uint32_t>(len - o < 4096 ? len - o : 4096), len) == kUnitOk);
        CHECK(unit_rule_region(len, len + 4096) == (len % 4096 ? kUnitPartial : kUnitOk));
        if (len) CHECK(unit_rule_region(len, len - 1) == kUnitBeyond);
    }
    CHECK(unit_rule_region(4096, 8192) == kUnitOk);
    CHECK(unit_rule_region(4097, 8192) == kUnitPartial);

    for (UnitBreach b : {kUnitOk, kUnitOffset, kUnitPartial, kUnitBeyond}) CHECK(unit_breach_text(b)[0] != 0);
    puts("ok");
    return 0;
}
