// cec_launchplan.hpp -- every decision of a kernel launch, as plain host arithmetic: the
// tiles of an extent, which kernel a pattern set takes (narrow, exact, a capacity rung),
// the workgroup split, the store policy and its write-through tail, the occupancy cap, the
// grid, the limits of one dispatch, and the check that an argument block serves its
// patterns.  One LaunchPlan per launch, filled by one pure function per kernel family;
// cec_runtime.hip's enqueue_launch turns it into the dispatch and the launch record.
//
// Standard library, cocytus_ec.h and cec_layout.hpp only -- no HIP type, no error
// reporting -- so tests/drain_c/launch_plan_main.cpp includes this very file under
// ASan + UBSan: these checks stand between a host mistake and a GPU fault.
#pragma once

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/cocytus_ec.h"
#include "cec_layout.hpp"

namespace cec {

// ============================================================== tiles
// Tiles of one extent end on 4 KiB boundaries of the arena offset, so interior
// tiles cover whole 128-B lines and only an extent's first / last tile shares a line
// with a neighbouring workgroup (ecalloc packs values at 16-B granularity; tiling
// from each value's start measured 4 % slower on the mixed workload).
static inline size_t tiles_of(uint64_t off, uint32_t len) {
    return len ? static_cast<size_t>((off % kTile + len + kTile - 1) / kTile) : 0;
}
static inline size_t append_tiles(Tile *t, uint64_t off, uint64_t src_off, uint32_t len,
                                  uint32_t pattern) {
    size_t n = 0;
    for (uint32_t o = 0; o < len;) {
        const uint32_t phase = static_cast<uint32_t>((off + o) % kTile);
        const uint32_t step = std::min<uint32_t>(kTile - phase, len - o);
        t[n++] = Tile{off + o, src_off + o, step, pattern};
        o += step;
    }
    return n;
}
// Full tiles whose arena offset sits on a 128-B line (the written side: a line
// written by two workgroups costs more than one read by two).
static inline int64_t count_line_tiles(const Tile *t, size_t n) {
    int64_t c = 0;
    for (size_t i = 0; i < n; ++i) c += t[i].len == kTile && (t[i].off & (kLineBytes - 1)) == 0;
    return c;
}

// ============================================================== which kernel
// The exact shapes (n_in, n_out, acc), X(N, L, A) for each -- the one list launch_exact's
// kernels and has_exact are both made from: encode / decode / residual / solve (no RMW,
// up to 8 inputs x 4 outputs), parity apply and region multiply-XOR (1 x 1 RMW),
// diff-update (2 inputs, M parity RMW outputs, optionally + install).
#define CEC_EXACT_WRITES(X, N) X(N, 1, kAccNone) X(N, 2, kAccNone) X(N, 3, kAccNone) X(N, 4, kAccNone)
#define CEC_EXACT_SHAPES(X)                                                                      \
    CEC_EXACT_WRITES(X, 1) CEC_EXACT_WRITES(X, 2) CEC_EXACT_WRITES(X, 3) CEC_EXACT_WRITES(X, 4)  \
    CEC_EXACT_WRITES(X, 5) CEC_EXACT_WRITES(X, 6) CEC_EXACT_WRITES(X, 7) CEC_EXACT_WRITES(X, 8)  \
    X(1, 1, kAccAll) X(2, 1, kAccAll) X(2, 2, kAccAll) X(2, 3, kAccAll) X(2, 4, kAccAll)         \
    X(2, 2, kAccAllButLast) X(2, 3, kAccAllButLast) X(2, 4, kAccAllButLast)

static bool has_exact(int n, int l, int acc) {
#define CEC_X(N, L, A) if (n == N && l == L && acc == A) return true;
    CEC_EXACT_SHAPES(CEC_X)
#undef CEC_X
    return false;
}

// The capacity ladder: a launch of nt inputs and lt outputs that has no exact kernel runs
// the capacity kernel of the next rung up, inputs 2 / 4 / 8 / 16 (the scrub kernels start
// at 4) and outputs 1 / 2 / 4.  CEC_CAPACITY_RUNGS(nt, lt, K) runs K(NT, LT) for that rung:
// capacity_rung names it (the launch record's nt / lt), the launchers run its kernel.
struct Capacity {
    int nt, lt;
};
#define CEC_LT_RUNGS(lt, NT, K)                  \
    if (lt <= 1) { K(NT, 1) }                    \
    else if (lt <= 2) { K(NT, 2) }               \
    else { K(NT, 4) }
#define CEC_CAPACITY_RUNGS_FROM_4(nt, lt, K)     \
    if (nt <= 4) { CEC_LT_RUNGS(lt, 4, K) }      \
    else if (nt <= 8) { CEC_LT_RUNGS(lt, 8, K) } \
    else { CEC_LT_RUNGS(lt, 16, K) }
#define CEC_CAPACITY_RUNGS(nt, lt, K)            \
    if (nt <= 2) { CEC_LT_RUNGS(lt, 2, K) }      \
    else { CEC_CAPACITY_RUNGS_FROM_4(nt, lt, K) }

static Capacity capacity_rung(int nt, int lt, bool from_4) {
#define CEC_RUNG(NT, LT) return {NT, LT};
    if (from_4) { CEC_CAPACITY_RUNGS_FROM_4(nt, lt, CEC_RUNG) }
    CEC_CAPACITY_RUNGS(nt, lt, CEC_RUNG)
#undef CEC_RUNG
}

// Shape class of the patterns a launch uses (`used`: pattern indices its tiles name;
// NULL = all): exact (n_in, n_out, acc) if they all agree.
static bool exact_shape(const std::vector<Pattern> &pats, const std::vector<char> *used, int *n, int *l,
                        int *acc) {
    const Pattern *p0 = nullptr;
    for (size_t i = 0; i < pats.size(); ++i) {
        if (used && !(*used)[i]) continue;
        const Pattern &p = pats[i];
        if (!p0) {
            p0 = &p;
            continue;
        }
        if (p.n_in != p0->n_in || p.n_out != p0->n_out) return false;
        for (int o = 0; o < p.n_out; ++o)
            if (p.out_mode[o] != p0->out_mode[o]) return false;
    }
    if (!p0) return false;
    int nx = 0;
    for (int o = 0; o < p0->n_out; ++o) nx += p0->out_mode[o] == kModeXor;
    if (nx == 0) *acc = kAccNone;
    else if (nx == p0->n_out) *acc = kAccAll;
    else if (nx == p0->n_out - 1 && p0->out_mode[p0->n_out - 1] == kModeWrite) *acc = kAccAllButLast;
    else return false;
    *n = p0->n_in;
    *l = p0->n_out;
    return true;
}

// The kernel a pattern set takes: capacities, LDS rows, and the exact shape if every
// pattern the launch uses has the same one.
struct LaunchShape {
    int nt = 1, lt = 0, max_rows = 0;
    bool exact = false;
    int en = 0, el = 0, eacc = 0;
    int streams = 0;  // 1 + the highest stream slot a used pattern names
};

static LaunchShape launch_shape(const std::vector<Pattern> &pats, const std::vector<char> *used) {
    LaunchShape sh;
    for (size_t i = 0; i < pats.size(); ++i) {
        if (used && !(*used)[i]) continue;
        sh.nt = std::max(sh.nt, pats[i].n_in);
        sh.lt = std::max(sh.lt, pats[i].n_out);
        sh.max_rows = std::max(sh.max_rows, pats[i].lds_rows);
        for (int j = 0; j < pats[i].n_in; ++j) sh.streams = std::max(sh.streams, pats[i].in_stream[j] + 1);
        for (int j = 0; j < pats[i].n_out; ++j) sh.streams = std::max(sh.streams, pats[i].out_stream[j] + 1);
    }
    sh.exact = exact_shape(pats, used, &sh.en, &sh.el, &sh.eacc);
    return sh;
}

enum KernelKind { kKindNarrow, kKindExact, kKindGeneric };
// (int on both sides: the C header's constants are an enum of its own)
static_assert(int(kKindNarrow) == CEC_KERNEL_NARROW && int(kKindExact) == CEC_KERNEL_EXACT &&
                  int(kKindGeneric) == CEC_KERNEL_GENERIC, "cec_launch_record::kind");
static_assert(int(kAccNone) == CEC_ACC_NONE && int(kAccAll) == CEC_ACC_ALL &&
                  int(kAccAllButLast) == CEC_ACC_ALL_BUT_LAST && int(kAccRuntime) == CEC_ACC_RUNTIME,
              "cec_launch_record::acc");
static_assert(kFlagSysRelease == CEC_LAUNCH_SYS_RELEASE && kFlagWriteThrough == CEC_LAUNCH_WRITE_THROUGH &&
                  kFlagWtTail == CEC_LAUNCH_WT_TAIL, "cec_launch_record::flags");

// The scrub's exact kernels: the codes the suite uses, when the launch holds the code's
// every parity (`whole_code`); every other scrub launch takes the capacity ladder's.
static bool scrub_exact(int k, int lt, bool whole_code) {
    return whole_code && ((k == 3 && lt == 2) || (k == 4 && lt == 2) || (k == 6 && lt == 3));
}

// ============================================================== the argument block
// The pattern set of one launch: where it lies on the device, and its host copy for the
// launch-time stream check.
struct Tables {
    const uint8_t *d;               // device blob: n_pats patterns, then the LDS engine's rows
    size_t n_pats;
    const Pattern *host;            // the same patterns on the host
    const std::vector<char> *used;  // which of them the launch's tiles name (NULL: all)
};

// Launch-time check of the argument block a kernel is passed: every stream slot a used
// pattern names must be one the block carries (below 2 for the narrow kernels, whose
// block is narrow_args' copy of the first two slots; below kMaxStreams otherwise) and
// hold a non-NULL base there.  Which arena the op meant for each slot is decided by the
// op itself (it fills the slots); this check catches a kernel choice or an argument block
// that cannot serve the patterns -- a slot the kernel's block does not have, or an empty
// one -- which would otherwise fault the GPU.  A failure is refused.
static bool stream_layout_ok(const uint8_t *const *bases, int slots, const Tables &tb) {
    for (size_t q = 0; q < tb.n_pats; ++q) {
        if (tb.used && (q >= tb.used->size() || !(*tb.used)[q])) continue;
        const Pattern &p = tb.host[q];
        for (int i = 0; i < p.n_in; ++i)
            if (p.in_stream[i] >= slots || !bases[p.in_stream[i]]) return false;
        for (int l = 0; l < p.n_out; ++l)
            if (p.out_stream[l] >= slots || !bases[p.out_stream[l]]) return false;
    }
    return true;
}

// ============================================================== knobs
// A byte count from the environment; a bad value is reported on stderr once and ignored.
static uint64_t parse_byte_count(const char *name, uint64_t dflt) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    // strtoull alone would take "-1" as 2^64 - 1 and skip leading blanks: a byte count is
    // digits only (decimal, 0x hex or 0 octal), in range
    char *end = nullptr;
    errno = 0;
    const unsigned long long v = (*e >= '0' && *e <= '9') ? strtoull(e, &end, 0) : 0;
    if (!(*e >= '0' && *e <= '9') || !end || *end || errno == ERANGE) {
        fprintf(stderr, "libcocytus_ec: %s=%s is not a byte count; using %llu\n", name, e,
                static_cast<unsigned long long>(dflt));
        return dflt;
    }
    return static_cast<uint64_t>(v);
}

enum { kStoreAuto = 0, kStoreNt = 1, kStoreWt = 2 };

// The measurement overrides of a process.  The library reads them from the environment
// once (Knobs::from_env, at load) and hands them to the planners: nothing below reads the
// environment, and a test states the knobs it means.
struct Knobs {
    int forced_split = -1;  // CEC_SPLIT_SHIFT=0..2 pins the workgroup split (-1: split_shift_for's rule)
    int store_policy = kStoreAuto;                  // CEC_STORE_POLICY=nt|wt|auto
    uint64_t wt_max_bytes = uint64_t(512) << 20;    // CEC_WT_MAX_BYTES (write_through)
    uint64_t wt_tail_bytes = uint64_t(96) << 20;    // CEC_WT_TAIL_BYTES; 0: no tail
    // Waves (work items) per workgroup of a digest launch, log2.  Four: a 256-lane workgroup
    // whose waves each take their own (tile, arena).  One-wave workgroups, the combine
    // kernels' split of full tiles, measured 10-12 % slower here (327,680 workgroups of
    // 4 KiB each against 81,920: DESIGN.md section 8).  CEC_DIGEST_WAVES_SHIFT=0..2 pins
    // another (measurement).
    uint32_t digest_waves_shift = 2;

    static int shift_from_env(const char *name, int dflt) {
        const char *e = getenv(name);
        return e && *e ? std::min(2, std::max(0, atoi(e))) : dflt;
    }
    static Knobs from_env() {
        Knobs k;
        k.forced_split = shift_from_env("CEC_SPLIT_SHIFT", -1);
        // An unknown value (e.g. "WT") is reported on stderr once and ignored (auto).
        const char *e = getenv("CEC_STORE_POLICY");
        if (!e || !*e || !strcmp(e, "auto")) k.store_policy = kStoreAuto;
        else if (!strcmp(e, "wt")) k.store_policy = kStoreWt;
        else if (!strcmp(e, "nt")) k.store_policy = kStoreNt;
        else fprintf(stderr, "libcocytus_ec: CEC_STORE_POLICY=%s is not nt, wt or auto; using auto\n", e);
        k.wt_max_bytes = parse_byte_count("CEC_WT_MAX_BYTES", k.wt_max_bytes);
        k.wt_tail_bytes = parse_byte_count("CEC_WT_TAIL_BYTES", k.wt_tail_bytes);
        k.digest_waves_shift = static_cast<uint32_t>(shift_from_env("CEC_DIGEST_WAVES_SHIFT", 2));
        return k;
    }
};

// ============================================================== split, stores, occupancy
// Workgroups per tile (log2).  Full tiles on 128-B lines stream fastest as four
// 64-lane workgroups (finer dispatch, every wave equal work).  A launch that is mostly
// small or line-misaligned tiles keeps one 256-lane workgroup per tile: splitting
// those multiplies empty workgroups and partial lines written by two workgroups
// (measured: DESIGN.md section 4).  CEC_SPLIT_SHIFT=0..2 pins the choice.
// `bases_or`: the OR of every stream base of the launch.
static uint32_t split_shift_for(const Knobs &kn, uintptr_t bases_or, uint64_t n_tiles, uint64_t n_line_tiles) {
    if (kn.forced_split >= 0) return static_cast<uint32_t>(kn.forced_split);
    const bool full = n_line_tiles * 4 >= n_tiles * 3;
    return full && (bases_or & (kLineBytes - 1)) == 0 ? 2u : 0u;
}

// Waves per CU a launch may hold (`cap`; 0 = as many as fit).  Fewer streaming waves per CU
// keep fewer HBM requests in flight; the cap is applied by sizing each workgroup's
// dynamic LDS so that only cap / (waves per workgroup) workgroups fit on a CU.
static size_t occupancy_lds(int cap, size_t lds_per_cu, uint32_t split_shift) {
    if (cap <= 0) return 0;
    const int waves_per_wg = (kBlock >> split_shift) / 64;
    const int wgs = std::max(1, cap / std::max(1, waves_per_wg));
    const size_t lds = lds_per_cu / static_cast<size_t>(wgs);
    return std::min<size_t>(65536, lds > 256 ? lds - 256 : 0);  // strictly below the boundary
}

// Store policy of a launch (kFlagWriteThrough).  Write-through (sc1) stores finish the
// launches of up to 512 MiB of streamed bytes sooner, non-temporal stores the larger
// ones.  RS(3,2) 4 KiB step, bench.py's strong-scaling shares, 3 processes per policy on
// one box (profiles/r03_evidence/store_policy_ab/): encode / decode us
//   8,192 stripes   nt 29.9-31.7 / 23.6-23.9   wt 27.5-28.6 / 22.3-22.6
//  16,384 stripes   nt 54.0-55.3 / 45.5-45.6   wt 53.4-54.0 / 41.0-41.6
//  32,768 stripes   nt 105.9-106.2 / 88.1-88.6 wt 112.5-112.7 / 81.1-81.8
//  65,536 stripes   nt 208.0-212.2 / 178.0-178.3  wt 223.3-224.8 / 184.8-186.1
// i.e. write-through wins at <= 335 MB (encode) and <= 537 MB (decode) per launch and
// loses at 671 MB (encode) and above.  Auto: write-through when the launch streams at
// most wt_max_bytes (reads + writes).  CEC_STORE_POLICY=nt|wt|auto and
// CEC_WT_MAX_BYTES override (measurement).
// A launch too large for write-through keeps non-temporal stores for its body and writes
// its last wt_tail_bytes (all outputs together) through.  Plain bench step (RS(3,2),
// 65,536 x 4 KiB, encode + rotating decode), 3 interleaved processes per tail on one box,
// GiB/s (profiles/store_tail_ab.md): no tail 2553-2581, 32 MiB 2568-2610, 64 MiB
// 2600-2634, 96 MiB 2643-2659, 128 MiB 2651-2666, 144 MiB 2647-2653, 160 MiB 2605-2612,
// 192 MiB 2520-2529, 256 MiB 2431-2449: a plateau from 96 to 144 MiB, the smallest of it
// taken.  The launch boundary is the same 5 us with and without (tools/trace_check.py):
// the gain is in the kernels' own time, the last writes of a launch being taken up on
// the memory side.  CEC_WT_TAIL_BYTES overrides (measurement); 0: no tail.
//
// Which work items of a launch store write-through: all (the kFlagWriteThrough launch),
// none, or those from `from` on.  `streamed`: the bytes the launch reads and writes.
struct StoreChoice {
    bool all;
    uint64_t from;  // kNoWtTail: none
};
static StoreChoice write_through(const Knobs &kn, uint64_t n_tiles, uint32_t split_shift, int lt, uint64_t streamed) {
    if (kn.store_policy != kStoreAuto) return {kn.store_policy == kStoreWt, kNoWtTail};
    if (streamed <= kn.wt_max_bytes) return {true, kNoWtTail};
    if (kn.wt_tail_bytes == 0 || lt <= 0) return {false, kNoWtTail};
    const uint64_t per_item = static_cast<uint64_t>(lt) * (kTile >> split_shift);  // bytes one work item writes
    const uint64_t items = kn.wt_tail_bytes / per_item + (kn.wt_tail_bytes % per_item != 0);
    const uint64_t n_work = n_tiles << split_shift;
    if (items >= n_work) return {true, kNoWtTail};  // the tail is the whole launch
    return {false, n_work - items};
}

// ============================================================== the plan of one launch
constexpr uint64_t kScrubMaxTiles = 0xFFFFFFFFull / kBlock;  // one dispatch: 64 GiB per arena
// One dispatch holds 2^32 - 1 work items; a digest launch has one wave per (tile, arena).
constexpr uint64_t kDigestMaxWork = 0xFFFFFFFFull / kBlock * (kBlock / 64);

// Why a planner plans no launch.  kPlanStreams and kPlanLayout are set by the enqueue
// routine, which alone sees the op's streams and patterns.
enum PlanRefusal {
    kPlanOk = 0,
    kPlanNothing,   // no tile, or no output: nothing to launch, and no error
    kPlanTooLarge,  // more work than one dispatch of this kernel holds
    kPlanNoKernel,  // a shape past the capacity kernels
    kPlanStreams,   // the op named more streams than an argument block has slots
    kPlanLayout,    // the argument block cannot serve the patterns (check_layout)
};

// One launch: what cec_last_launch reports of it, and the workgroup size.
struct LaunchPlan {
    int kind = -1;       // CEC_KERNEL_*
    int nt = 0, lt = 0;  // the kernel's capacity (exact and narrow kernels: the shape itself)
    int acc = kAccNone, engine = CEC_ENGINE_PERM;
    uint32_t split_shift = 0, flags = 0, grid = 0;
    uint64_t n_tiles = 0;
    size_t lds_bytes = 0;  // dynamic LDS (LDS engine: the largest pattern's rows; the occupancy cap)
    uint64_t wt_from = kNoWtTail;
    uint32_t block = kBlock;  // lanes per workgroup
    PlanRefusal refusal = kPlanOk;
};

static LaunchPlan plan_start(int kind, uint64_t n_tiles, uint64_t max_tiles) {
    LaunchPlan p;
    p.kind = kind;
    p.n_tiles = n_tiles;
    p.refusal = n_tiles == 0 ? kPlanNothing : n_tiles > max_tiles ? kPlanTooLarge : kPlanOk;
    return p;
}

// A combine launch.  Which kernel runs: the exact-shape one if the shape has an
// instantiation, the narrow two-slot one for 1 x 1 launches over slots 0 and 1, else a
// capacity kernel.  `waves_per_cu`, `lds_per_cu`: the occupancy cap and the device's LDS.
static LaunchPlan plan_combine(const LaunchShape &sh, uint64_t n_tiles, uint64_t n_line_tiles, uintptr_t bases_or,
                               bool lds, uint32_t flags, const Knobs &kn, int waves_per_cu, size_t lds_per_cu) {
    LaunchPlan p = plan_start(kKindGeneric, n_tiles, 0xFFFFFFFFull);
    if (p.refusal == kPlanOk && sh.lt == 0) p.refusal = kPlanNothing;
    if (p.refusal == kPlanOk && (sh.nt > kPatN || sh.lt > kPatL)) p.refusal = kPlanNoKernel;
    if (p.refusal != kPlanOk) return p;
    const bool exact_k = sh.exact && has_exact(sh.en, sh.el, sh.eacc);
    if (exact_k)
        p.kind = sh.en == 1 && sh.el == 1 && sh.streams <= kNarrowStreams && (sh.eacc == kAccAll || sh.eacc == kAccNone)
                     ? kKindNarrow
                     : kKindExact;
    const Capacity cap = exact_k ? Capacity{sh.en, sh.el} : capacity_rung(sh.nt, sh.lt, false);
    p.nt = cap.nt;
    p.lt = cap.lt;
    p.acc = exact_k ? sh.eacc : static_cast<int>(kAccRuntime);
    p.engine = lds ? CEC_ENGINE_LDS : CEC_ENGINE_PERM;
    // One workgroup per (part of a) tile, dispatched in tile order, so the set of
    // tiles in flight is a contiguous window of the arenas (measured 5-12 % over a
    // persistent grid-stride grid: DESIGN.md).  The LDS engine stages its pattern's
    // product rows per workgroup (512 B for an RS(3,2) encode, from L2).
    p.split_shift = split_shift_for(kn, bases_or, n_tiles, n_line_tiles);
    p.block = kBlock >> p.split_shift;
    // The store policy.  A tail needs the full block's wt_from and the PERM engine's store
    // branch: the narrow and the LDS engine's kernels have neither, and get no tail.
    const StoreChoice wt = write_through(kn, n_tiles, p.split_shift, sh.lt,
                                         n_tiles * kTile * static_cast<uint64_t>(sh.nt + sh.lt));
    p.wt_from = p.kind == kKindNarrow || lds ? kNoWtTail : wt.from;
    p.flags = flags | (wt.all ? kFlagWriteThrough : 0u) | (p.wt_from != kNoWtTail ? kFlagWtTail : 0u);
    p.lds_bytes = std::max(lds ? static_cast<size_t>(sh.max_rows) * 256 : 0,
                           occupancy_lds(waves_per_cu, lds_per_cu, p.split_shift));
    // A dispatch holds at most 2^32 - 1 work items per dimension: past that (more than
    // 64 GiB of tiles per stream) workgroups walk the rest grid-stride.
    p.grid = static_cast<uint32_t>(std::min<uint64_t>(n_tiles << p.split_shift, 0xFFFFFFFFull / p.block));
    return p;
}

// A scrub launch over k data and lt parity streams: one workgroup per (part of a) tile and
// no grid-stride, so at most kScrubMaxTiles tiles.
static LaunchPlan plan_scrub(int k, int lt, bool whole_code, uint64_t n_tiles, uint64_t n_line_tiles,
                             uintptr_t bases_or, const Knobs &kn, int waves_per_cu, size_t lds_per_cu) {
    LaunchPlan p = plan_start(CEC_KERNEL_SCRUB, n_tiles, kScrubMaxTiles);
    if (p.refusal != kPlanOk) return p;
    const Capacity cap = scrub_exact(k, lt, whole_code) ? Capacity{k, lt} : capacity_rung(k, lt, true);
    p.nt = cap.nt;
    p.lt = cap.lt;
    p.acc = kAccAll;
    p.split_shift = split_shift_for(kn, bases_or, n_tiles, n_line_tiles);
    p.block = kBlock >> p.split_shift;
    p.lds_bytes = occupancy_lds(waves_per_cu, lds_per_cu, p.split_shift);
    p.grid = static_cast<uint32_t>(n_tiles << p.split_shift);
    return p;
}

// A digest launch over n arenas: one wave per (tile, arena), 2^digest_waves_shift a workgroup.
static LaunchPlan plan_digest(int n, uint64_t n_tiles, const Knobs &kn) {
    LaunchPlan p = plan_start(CEC_KERNEL_DIGEST, n_tiles, kDigestMaxWork / static_cast<uint64_t>(std::max(n, 1)));
    if (p.refusal != kPlanOk) return p;
    p.nt = n;
    const uint64_t per_wg = uint64_t(1) << kn.digest_waves_shift;
    p.block = 64u << kn.digest_waves_shift;
    p.grid = static_cast<uint32_t>((n_tiles * static_cast<uint64_t>(n) + per_wg - 1) / per_wg);
    return p;
}

// A digest update: one wave per tile, four per workgroup.
static LaunchPlan plan_digest_update(uint64_t n_tiles) {
    LaunchPlan p = plan_start(CEC_KERNEL_DIGEST_UPDATE, n_tiles, kDigestMaxWork);
    if (p.refusal != kPlanOk) return p;
    p.nt = 1;
    p.acc = kAccAll;
    p.grid = static_cast<uint32_t>((n_tiles + 3) / 4);
    return p;
}

// A digest set (the SET path's digest launch): one wave per tile, four per workgroup; each
// wave reads two sources, the staged value and the data arena's old bytes.
static LaunchPlan plan_digest_set(uint64_t n_tiles) {
    LaunchPlan p = plan_start(CEC_KERNEL_DIGEST_SET, n_tiles, kDigestMaxWork);
    if (p.refusal != kPlanOk) return p;
    p.nt = 2;
    p.acc = kAccAll;
    p.grid = static_cast<uint32_t>((n_tiles + 3) / 4);
    return p;
}

// A digest-emitting combination (cec_encode_digests, cec_decode_digests): one wave per whole
// unit, four per workgroup, no grid-stride.  `n_in`: the most inputs a pattern of the launch
// has (the kernel walks them in a loop: no input capacity); `lt`: the most outputs, run by the
// output capacity 1, 2 or 4 above it (a launch that only digests its inputs has lt = 0 and runs
// capacity 1).
static int combine_digest_capacity(int lt) { return lt <= 1 ? 1 : lt <= 2 ? 2 : 4; }
static LaunchPlan plan_combine_digest(int n_in, int lt, uint64_t n_tiles) {
    LaunchPlan p = plan_start(CEC_KERNEL_COMBINE_DIGEST, n_tiles, kDigestMaxWork);
    if (p.refusal == kPlanOk && (n_in < 0 || n_in > kPatN || lt < 0 || lt > kPatL)) p.refusal = kPlanNoKernel;
    if (p.refusal != kPlanOk) return p;
    p.nt = n_in;
    p.lt = combine_digest_capacity(lt);
    p.grid = static_cast<uint32_t>((n_tiles + 3) / 4);
    return p;
}

// The unit rule of the digest-emitting ops.  The digest of a partly written unit cannot be
// formed without its old bytes, so every tile of such an op is a whole 4 KiB unit at a 4 KiB
// arena offset; the one exception is the arena's own ragged last unit, a tile shorter than
// 4 KiB that ends exactly at arena_len (its digest is that of the bytes zero-padded, as
// cec_digest_region forms it).  No tile ends beyond arena_len.  Tiles are append_tiles' pieces
// of the extents, so the rule on them is the rule on the extents: an extent at a 4 KiB offset
// yields whole units and at most a short last tile, any other offset a misplaced first tile.
enum UnitBreach {
    kUnitOk = 0,
    kUnitOffset,   // the tile does not start on a 4 KiB arena boundary
    kUnitPartial,  // shorter than a unit and not the end of the arena
    kUnitBeyond,   // ends beyond arena_len
};
static UnitBreach unit_rule_tile(uint64_t off, uint32_t len, uint64_t arena_len) {
    if (off % kTile != 0) return kUnitOffset;
    if (off > arena_len || len > arena_len - off) return kUnitBeyond;
    if (len != kTile && off + len != arena_len) return kUnitPartial;
    return kUnitOk;
}
// The first tile that breaks the rule (*bad), or kUnitOk.
static UnitBreach unit_rule_tiles(const Tile *t, size_t n, uint64_t arena_len, size_t *bad) {
    for (size_t i = 0; i < n; ++i)
        if (const UnitBreach b = unit_rule_tile(t[i].off, t[i].len, arena_len)) {
            if (bad) *bad = i;
            return b;
        }
    return kUnitOk;
}
// The implicit region [0, len) of an arena of arena_len bytes: whole units, and a short last
// one only where the region is the whole arena.
static UnitBreach unit_rule_region(uint64_t len, uint64_t arena_len) {
    if (len > arena_len) return kUnitBeyond;
    if (len % kTile != 0 && len != arena_len) return kUnitPartial;
    return kUnitOk;
}
static const char *unit_breach_text(UnitBreach b) {
    switch (b) {
    case kUnitOffset: return "does not start on a 4096-byte arena boundary";
    case kUnitPartial: return "is a partial unit that does not end at arena_len";
    case kUnitBeyond: return "ends beyond arena_len";
    default: return "is a whole unit";
    }
}

// A digest check of lt parities against k data digests: one lane per unit, as many units
// as a scrub report holds tiles.
static LaunchPlan plan_digest_check(int k, int lt, uint64_t n_units) {
    LaunchPlan p = plan_start(CEC_KERNEL_DIGEST_CHECK, n_units, kScrubMaxTiles);
    if (p.refusal != kPlanOk) return p;
    const Capacity cap = capacity_rung(k, lt, true);
    p.nt = cap.nt;
    p.lt = cap.lt;
    p.acc = kAccAll;
    p.grid = static_cast<uint32_t>((n_units + kBlock - 1) / kBlock);
    return p;
}

// The layout check of a planned launch: `bases` is the stream array of the argument block
// its kernel is passed, which has as many slots as the kernel's kind says.
static void check_layout(LaunchPlan &p, const uint8_t *const *bases, const Tables &tb) {
    const int slots = p.kind == kKindNarrow ? kNarrowStreams
                      : p.kind <= kKindGeneric || p.kind == CEC_KERNEL_COMBINE_DIGEST ? kMaxStreams
                                                                                      : kScrubStreams;
    if (p.refusal == kPlanOk && !stream_layout_ok(bases, slots, tb)) p.refusal = kPlanLayout;
}

}  // namespace cec
