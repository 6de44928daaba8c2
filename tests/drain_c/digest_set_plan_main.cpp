// plan_digest_set of cec_launchplan.hpp against its documented rule, restated here: one wave
// per tile and four waves per workgroup, so grid = ceil(tiles / 4); at most 67,108,860 tiles
// in one dispatch; the launch record is kind 7, 2 x 0, every destination read-modify-write,
// PERM, no split, no flags, no dynamic LDS.  Includes the shipped header; built with
// ASan + UBSan by tests/test_digest_set.py.  Prints "ok".
#include <cstdio>
#include <cstdlib>

#include "cec_launchplan.hpp"

using namespace cec;

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            exit(1);                                                  \
        }                                                             \
    } while (0)

static void check_record(const LaunchPlan &p, uint64_t tiles, uint32_t grid) {
    CHECK(p.refusal == kPlanOk);
    CHECK(p.kind == 7 && p.kind == CEC_KERNEL_DIGEST_SET);
    CHECK(p.nt == 2 && p.lt == 0);
    CHECK(p.acc == CEC_ACC_ALL);
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

int main() {
    const uint64_t kMax = 67108860;  // (2^32 - 1) / 256 workgroups of four waves
    CHECK(kDigestMaxWork == kMax);

    const LaunchPlan none = plan_digest_set(0);
    CHECK(none.refusal == kPlanNothing && none.grid == 0 && none.kind == CEC_KERNEL_DIGEST_SET);

    check_record(plan_digest_set(1), 1, 1);
    check_record(plan_digest_set(3), 3, 1);
    check_record(plan_digest_set(4), 4, 1);
    check_record(plan_digest_set(5), 5, 2);
    check_record(plan_digest_set(14), 14, 4);
    check_record(plan_digest_set(65536), 65536, 16384);
    check_record(plan_digest_set(kMax), kMax, 16777215);

    const LaunchPlan big = plan_digest_set(kMax + 1);
    CHECK(big.refusal == kPlanTooLarge && big.grid == 0);
    CHECK(plan_digest_set(~uint64_t(0)).refusal == kPlanTooLarge);

    // the same limits and grid as the digest update's
    for (uint64_t n : {uint64_t(0), uint64_t(1), uint64_t(5), kMax, kMax + 1}) {
        const LaunchPlan a = plan_digest_set(n), b = plan_digest_update(n);
        CHECK(a.refusal == b.refusal && a.grid == b.grid && a.block == b.block);
    }
    printf("ok\n");
    return 0;
}
