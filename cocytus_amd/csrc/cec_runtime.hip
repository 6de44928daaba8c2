// cec_runtime.hip -- libcocytus_ec.so: the C-ABI of the MI355X erasure-coding path.
//
// Exports (a) the three Jerasure 2.x symbols Cocytus links:
//   galois_w08_region_multiply             (memcached.c:2681,5611,7764,7918; recovery.c:91,123)
//   reed_sol_big_vandermonde_distribution_matrix   (memcached.c:6845)
//   jerasure_invert_matrix                 (memcached.c:7907)
// plus a few same-header helpers, and (b) the batched device API of cocytus_ec.h.
// Every byte of region arithmetic runs in the HIP kernels of cec_kernels.hpp; the
// host side only builds coefficient tables, tile work-lists and launches.  There is
// no CPU fallback: without a gfx950 device the batched API returns CEC_ENODEV and
// the void Jerasure entry point aborts with a message.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cocytus_ec.h"
#include "../../include/galois.h"
#include "../../include/jerasure.h"
#include "../../include/reed_sol.h"
#include "cec_hostplan.hpp"
#include "cec_kernels.hpp"
#include "cec_launchplan.hpp"
#include "cec_poolbook.hpp"
#include "gf256.hpp"

#define CEC_API extern "C" __attribute__((visibility("default")))

using namespace cec;

static_assert(sizeof(Tile) == sizeof(cec_extent), "tile layout");
static_assert(CEC_MAX_K <= kPatN, "k capacity");

// ============================================================== errors
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(CEC_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                        __FILE__, __LINE__);                                               \
    } while (0)

[[noreturn]] static void die(const char *what) {
    fprintf(stderr, "libcocytus_ec: fatal: %s\n", what);
    fflush(stderr);
    abort();
}

// ============================================================== device state
struct DevInfo {
    std::once_flag once;
    int status = CEC_ENODEV;
    int cus = 256;
    size_t lds_per_cu = 160 * 1024;  // gfx950
    char msg[256] = "";
};
static DevInfo g_dev[64];
static std::atomic<int> g_engine{CEC_ENGINE_AUTO};

// The engine an op runs with, read once per op (its tables and its kernel must agree):
// the process-wide setting, or under AUTO the LDS engine only where it led PERM by more
// than 2 % on the median of the recorded boxes -- `lds_op`: a decode of values of 64 KiB
// and more -- and PERM for every other op (cocytus_ec.h; DESIGN.md §4 "Engine per op").
// Recorded per thread for cec_last_engine().
static thread_local int t_last_engine = -1;
static int op_engine(bool lds_op) {
    const int e = g_engine.load();
    const int r = e == CEC_ENGINE_AUTO ? (lds_op ? CEC_ENGINE_LDS : CEC_ENGINE_PERM) : e;
    t_last_engine = r;
    return r;
}

static int current_device(int *dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(CEC_ENODEV, "no HIP device visible (libcocytus_ec has no CPU fallback)");
    }
    HIP_TRY(hipGetDevice(dev));
    if (*dev < 0 || *dev >= 64) return fail(CEC_ENODEV, "device ordinal %d out of range", *dev);
    DevInfo &d = g_dev[*dev];
    std::call_once(d.once, [&] {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, *dev) != hipSuccess) {
            snprintf(d.msg, sizeof d.msg, "hipGetDeviceProperties(%d) failed", *dev);
            return;
        }
        if (strncmp(p.gcnArchName, "gfx950", 6) != 0) {
            snprintf(d.msg, sizeof d.msg, "device %d is %s, libcocytus_ec is built for gfx950",
                     *dev, p.gcnArchName);
            return;
        }
        d.cus = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
        if (p.maxSharedMemoryPerMultiProcessor > 0) d.lds_per_cu = p.maxSharedMemoryPerMultiProcessor;
        d.status = CEC_OK;
    });
    if (d.status != CEC_OK) return fail(d.status, "%s", d.msg);
    return CEC_OK;
}

#include "cec_cache.inc"

static Pattern blank_pattern() {
    Pattern p;
    memset(&p, 0, sizeof p);
    return p;
}

static void set_coef(Pattern &p, int l, int i, int c, int engine) {
    c &= 0xFF;
    p.coef[l][i] = static_cast<uint8_t>(c);
    if (engine != CEC_ENGINE_LDS) {
        const PermTab t = make_perm_tab(c);
        for (int w = 0; w < 5; ++w) p.tab[l][i][w] = t.w[w];
    }
}

// LDS engine: one 256-B product row per distinct coefficient c >= 2 of the pattern,
// row_c[x] = exp[log x + log c] (0 for x = 0), appended to `rows`; the kernel stages
// the pattern's rows into LDS and looks up one byte per byte (cec_kernels.hpp).
static void assign_rows(Pattern &p, std::vector<uint8_t> &rows) {
    int row_of[256];
    for (int &r : row_of) r = -1;
    const size_t base = rows.size() / 256;
    int nr = 0;
    for (int l = 0; l < p.n_out; ++l)
        for (int i = 0; i < p.n_in; ++i) {
            const int c = p.coef[l][i];
            if (c < 2) continue;  // 0 and 1 are uniform branches, no table
            if (row_of[c] < 0) {
                row_of[c] = nr++;
                for (int x = 0; x < 256; ++x)
                    rows.push_back(x ? kGf.exp[kGf.log[x] + kGf.log[c]] : 0);
            }
            p.tab[l][i][0] = static_cast<uint32_t>(row_of[c]) * 256u;
        }
    p.lds_rows = nr;
    p.lds_row_base = static_cast<int32_t>(base);
}

// ============================================================== launch
// The template dispatch of a planned launch (cec_launchplan.hpp): grid, workgroup size and
// dynamic LDS are the plan's.
template <int NT, int LT, class Eng, int kAcc, bool kExact, int S = kMaxStreams, bool kSysRel = false>
static void launch_k(const CombineArgsN<S> &a, const LaunchPlan &lp, hipStream_t s) {
    hipLaunchKernelGGL((combine_kernel<NT, LT, Eng, kAcc, kExact, S, kSysRel>), dim3(lp.grid), dim3(lp.block),
                       lp.lds_bytes, s, a);
}

// The 1 x 1 shapes (region multiply-XOR / write, parity apply) with the two-slot
// arguments, for launches whose patterns use slots 0 and 1 only.
static CombineArgsN<kNarrowStreams> narrow_args(const CombineArgs &w) {
    CombineArgsN<kNarrowStreams> a;
    memset(&a, 0, sizeof a);
    for (int i = 0; i < kNarrowStreams; ++i) a.base[i] = w.base[i];
    a.tiles = w.tiles;
    a.patterns = w.patterns;
    a.rows = w.rows;
    a.implicit_len = w.implicit_len;
    a.n_tiles = w.n_tiles;
    a.split_shift = w.split_shift;
    a.grid = w.grid;
    a.flags = w.flags;
    return a;
}

template <class Eng>
static bool launch_narrow(const CombineArgsN<kNarrowStreams> &a, const LaunchPlan &lp, hipStream_t s) {
    const bool rel = (a.flags & kFlagSysRelease) != 0;
    if (lp.acc == kAccAll && rel) launch_k<1, 1, Eng, kAccAll, true, kNarrowStreams, true>(a, lp, s);
    else if (lp.acc == kAccAll) launch_k<1, 1, Eng, kAccAll, true, kNarrowStreams>(a, lp, s);
    else if (lp.acc == kAccNone && rel) launch_k<1, 1, Eng, kAccNone, true, kNarrowStreams, true>(a, lp, s);
    else if (lp.acc == kAccNone) launch_k<1, 1, Eng, kAccNone, true, kNarrowStreams>(a, lp, s);
    else return false;
    return true;
}

// One kernel per exact shape of CEC_EXACT_SHAPES, the list has_exact is made from.
template <class Eng>
static bool launch_exact(const CombineArgs &a, const LaunchPlan &lp, hipStream_t s) {
#define CEC_X(N, L, A)                                    \
    if (lp.nt == N && lp.lt == L && lp.acc == A) {        \
        launch_k<N, L, Eng, A, true>(a, lp, s);           \
        return true;                                      \
    }
    CEC_EXACT_SHAPES(CEC_X)
#undef CEC_X
    return false;
}

// Capacity kernels for every shape without an exact one (guarded, per-pattern counts and
// modes): the plan's rung of the capacity ladder.
template <class Eng>
static void launch_generic(const CombineArgs &a, const LaunchPlan &lp, hipStream_t s) {
#define CEC_G(NT, LT)                                       \
    launch_k<NT, LT, Eng, kAccRuntime, false>(a, lp, s);    \
    return;
    CEC_CAPACITY_RUNGS(lp.nt, lp.lt, CEC_G)
#undef CEC_G
}

#include "cec_combo.inc"

// ============================================================== plans
struct cec_plan {
    int device = -1;
    int n_ext = 0;
    int64_t n_tiles = 0;
    uint64_t total = 0;
    bool overlap = false;
    int64_t n_line_tiles = 0;   // full kTile tiles at a 128-B aligned arena offset
    Tile *d_tiles = nullptr;    // from dev_cache() (NULL: the empty plan)
    uint32_t max_pattern = 0;       // largest extent pattern (per-op index validation)
    uint64_t max_end = 0;           // largest off + len of a non-empty extent (saturating) ...
    int max_end_ext = -1;           // ... and the first extent that reaches it
    std::vector<Tile> h_tiles;      // kept alive for the async upload
    mutable Tracker uses;           // the streams of the tile upload and of every launch
};

CEC_API int cec_plan_destroy(cec_plan *p) {
    if (!p) return CEC_OK;
    int rc = CEC_OK;
    // only this plan's own work: its upload and its launches on every stream used
    if (hipError_t e = p->uses.wait(p->device); e != hipSuccess)
        rc = fail(CEC_EHIP, "cec_plan_destroy: a launch of this plan failed: %s", hipGetErrorString(e));
    dev_cache().release(p->device, p->d_tiles, sizeof(Tile) * p->n_tiles);  // (NULL: nothing)
    delete p;
    return rc;
}

// The caller is destroying `stream`: wait for this plan's work on it and stop tracking it
// (per-connection streams: the tracked list stays bounded by the streams alive).
CEC_API int cec_plan_release_stream(cec_plan *p, void *stream) {
    if (!p) return fail(CEC_EINVAL, "cec_plan_release_stream: plan is NULL");
    if (hipError_t e = p->uses.release(p->device, static_cast<hipStream_t>(stream)); e != hipSuccess)
        return fail(CEC_EHIP, "cec_plan_release_stream: %s", hipGetErrorString(e));
    return CEC_OK;
}
CEC_API int cec_plan_tracked_streams(const cec_plan *p) { return p ? static_cast<int>(p->uses.size()) : 0; }

CEC_API int cec_plan_create(cec_plan **out, const cec_extent *ext, int n, void *stream) {
    if (!out || n < 0 || (n > 0 && !ext)) return fail(CEC_EINVAL, "cec_plan_create: bad args");
    *out = nullptr;
    int dev;
    if (int r = current_device(&dev)) return r;
    cec_plan *p = new (std::nothrow) cec_plan;
    if (!p) return fail(CEC_ENOMEM, "cec_plan_create: host allocation");
    p->device = dev;
    p->n_ext = n;
    for (int e = 0; e < n; ++e) {
        p->max_pattern = std::max(p->max_pattern, ext[e].pattern);
        if (!ext[e].len) continue;
        const uint64_t end = ext[e].off > UINT64_MAX - ext[e].len ? UINT64_MAX : ext[e].off + ext[e].len;
        if (p->max_end_ext < 0 || end > p->max_end) {
            p->max_end = end;
            p->max_end_ext = e;
        }
    }
    size_t total_tiles = 0;
    for (int e = 0; e < n; ++e) total_tiles += tiles_of(ext[e].off, ext[e].len);
    p->h_tiles.resize(total_tiles);
    size_t nt = 0;
    for (int e = 0; e < n; ++e) {
        p->total += ext[e].len;
        nt += append_tiles(p->h_tiles.data() + nt, ext[e].off, ext[e].src_off, ext[e].len, ext[e].pattern);
    }
    if (p->h_tiles.size() > 0xFFFFFFFFull) {
        delete p;
        return fail(CEC_EINVAL, "cec_plan_create: more than 2^32 tiles");
    }
    p->n_tiles = static_cast<int64_t>(p->h_tiles.size());
    p->n_line_tiles = count_line_tiles(p->h_tiles.data(), p->h_tiles.size());
    {   // overlap of [off, off+len) among non-empty extents
        std::vector<std::pair<uint64_t, uint64_t>> r;
        r.reserve(n);
        for (int e = 0; e < n; ++e)
            if (ext[e].len) r.emplace_back(ext[e].off, ext[e].off + ext[e].len);
        std::sort(r.begin(), r.end());
        for (size_t i = 1; i < r.size(); ++i)
            if (r[i].first < r[i - 1].second) { p->overlap = true; break; }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p->n_tiles > 0) {
        const size_t bytes = sizeof(Tile) * p->n_tiles;
        p->d_tiles = static_cast<Tile *>(dev_cache().acquire(dev, bytes));
        if (!p->d_tiles) {
            delete p;
            return fail(CEC_ENOMEM, "cec_plan_create: %zu bytes of tiles", bytes);
        }
        if (hipMemcpyAsync(p->d_tiles, p->h_tiles.data(), bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
            (void)hipGetLastError();
            cec_plan_destroy(p);
            return fail(CEC_EHIP, "cec_plan_create: tile upload failed");
        }
        p->uses.note(s);  // destroy waits for the upload too
    }
    *out = p;
    return CEC_OK;
}

CEC_API int cec_plan_num_extents(const cec_plan *p) { return p ? p->n_ext : 0; }
CEC_API int64_t cec_plan_num_tiles(const cec_plan *p) { return p ? p->n_tiles : 0; }
CEC_API uint64_t cec_plan_total_bytes(const cec_plan *p) { return p ? p->total : 0; }

// What one launch walks: a run of device tiles, or (tiles == NULL) the implicit 4 KiB
// tiling of a region.  Made in one of the three ways below and no other, so the tile
// count and the full-line-tile count -- which alone decides the workgroup split,
// split_shift_for -- always come with the tiles.
struct TileSource {
    const Tile *tiles = nullptr;  // device address; NULL: the region [0, implicit_len)
    uint64_t n_tiles = 0;
    uint64_t n_line_tiles = 0;    // full kTile tiles at a 128-B aligned offset
    uint64_t implicit_len = 0;
    Tracker *uses = nullptr;      // a plan's streams, for its destroy; NULL for windows and
                                  // regions, whose owners track their own calls

    // A plan's tiles, on the device the plan was built on.
    static int of_plan(const cec_plan *plan, int dev, TileSource *out) {
        if (plan->device != dev)
            return fail(CEC_EINVAL, "plan built on device %d used on device %d", plan->device, dev);
        *out = {plan->d_tiles, static_cast<uint64_t>(plan->n_tiles), static_cast<uint64_t>(plan->n_line_tiles), 0,
                &plan->uses};
        return CEC_OK;
    }
    // The region [0, len): every tile counts as a full line tile (at most the last is short).
    static int of_region(uint64_t len, TileSource *out) {
        const uint64_t n = (len + kTile - 1) / kTile;
        if (n > 0xFFFFFFFFull) return fail(CEC_EINVAL, "region too large");
        *out = {nullptr, n, n, len, nullptr};
        return CEC_OK;
    }
    // n tiles of an op's own tile buffer: d on the device, h the same tiles on the host.
    static TileSource window(const Tile *d, const Tile *h, size_t n) {
        return {d, n, static_cast<uint64_t>(count_line_tiles(h, n)), 0, nullptr};
    }
    // ... whose tiles the caller knows to be whole 4 KiB units at 4 KiB offsets.
    static TileSource whole_units(const Tile *d, size_t n) { return {d, n, n, 0, nullptr}; }
};

// The tile list of an op whose items run in overlap waves, one launch per wave: items
// are added in wave order into the caller's host tile buffer (which must hold them),
// and each wave's range is kept for its launch window.
struct WaveTiles {
    Tile *h;
    size_t n = 0;               // tiles so far
    std::vector<size_t> first;  // first tile of each wave begun
    int cur = -1;
    explicit WaveTiles(Tile *host) : h(host) {}
    void begin_wave() { first.push_back(n); }
    void enter(int wave) {  // begin_wave() whenever the items' wave changes
        if (wave != cur) begin_wave();
        cur = wave;
    }
    void add(uint64_t off, uint64_t src_off, uint32_t len, uint32_t pattern) {
        n += append_tiles(h + n, off, src_off, len, pattern);
    }
    int waves() const { return static_cast<int>(first.size()); }
    // Every tile added so far, whatever its wave (for a launch whose tiles may overlap).
    TileSource all(const Tile *d) const { return TileSource::window(d, h, n); }
    // Wave w's launch, d being the device address of h; n_tiles == 0: nothing to launch.
    TileSource window(int w, const Tile *d) const {
        const size_t lo = first[w], hi = w + 1 < waves() ? first[w + 1] : n;
        return TileSource::window(d + lo, h + lo, hi - lo);
    }
};

// The measurement overrides in force (cec_launchplan.hpp), read from the environment once.
static const Knobs g_knobs = Knobs::from_env();

// The occupancy cap (occupancy_lds).  CEC_WAVES_PER_CU overrides it (measurement).
static std::atomic<int> g_waves_per_cu{[] {
    const char *e = getenv("CEC_WAVES_PER_CU");
    return e && *e ? std::max(0, atoi(e)) : 0;
}()};
static int waves_per_cu_cap() { return g_waves_per_cu.load(std::memory_order_relaxed); }

// The store policy in force (tests: every kernel kind runs under each).
CEC_API int cec_internal_store_policy(uint64_t *wt_max_bytes) {
    if (wt_max_bytes) *wt_max_bytes = g_knobs.wt_max_bytes;
    return g_knobs.store_policy;
}
// Test hook: write_through's choice for a launch of n_tiles tiles, lt outputs, `streamed`
// bytes.  Returns 0 none, 1 a tail from *wt_from, 2 all.
CEC_API int cec_internal_wt_from(uint64_t n_tiles, uint32_t split_shift, int lt, uint64_t streamed,
                                 uint64_t *wt_tail_bytes, uint64_t *wt_from) {
    if (split_shift > 2 || n_tiles > 0xFFFFFFFFull) return fail(CEC_EINVAL, "cec_internal_wt_from: bad args");
    const StoreChoice c = write_through(g_knobs, n_tiles, split_shift, lt, streamed);
    if (wt_tail_bytes) *wt_tail_bytes = g_knobs.wt_tail_bytes;
    if (wt_from) *wt_from = c.from;
    return c.all ? 2 : c.from != kNoWtTail ? 1 : 0;
}

// The calling thread's last enqueued kernel launch (cec_last_launch).  record_launch is
// the one place that writes it, and enqueue_launch its one caller.
static thread_local cec_launch_record t_last_launch = {0, -1, 0, 0, -1, -1, 0, 0, 0, 0, 0, kNoWtTail};

static void record_launch(const LaunchPlan &lp) {
    t_last_launch = {t_last_launch.seq + 1, lp.kind, lp.nt, lp.lt, lp.acc, lp.engine, lp.split_shift, lp.flags,
                     lp.grid, lp.n_tiles, lp.lds_bytes, lp.wt_from};
}

CEC_API int cec_last_launch(cec_launch_record *out) {
    if (!out) return fail(CEC_EINVAL, "cec_last_launch: out is NULL");
    *out = t_last_launch;
    return CEC_OK;
}

// Test hook (cec_internal_fail_launch): the calling thread's next `after` launches run, the
// one after them is refused as a HIP failure, then the hook disarms.  -1: off.
// Counted by enqueue_launch (launch_countdown) for run_combine, scrub_launch and the digest
// launches, before anything is pinned.
static thread_local int t_fail_after = -1;
CEC_API int cec_internal_fail_launch(int after) {
    t_fail_after = after < 0 ? -1 : after;
    return CEC_OK;
}
static int launch_countdown() {
    if (t_fail_after == 0) {
        t_fail_after = -1;
        return fail(CEC_EHIP, "injected launch failure (cec_internal_fail_launch)");
    }
    if (t_fail_after > 0) --t_fail_after;
    return CEC_OK;
}

// The device copy of a pattern set from the coefficient cache, for a launch on stream s:
// patterns and the LDS engine's product rows (NULL: none) are one blob, rows after the
// patterns (16-B aligned: sizeof(Pattern) is a multiple of 16), and the blob's bytes are its
// cache key.  *entry is pinned against eviction until pattern_done, which the caller calls
// once its launch is enqueued (eviction synchronises the device).
static int pattern_tables(int dev, const Pattern *pats, size_t n_pats, const std::vector<uint8_t> *rows,
                          hipStream_t s, PatEntry **entry) {
    std::string key(reinterpret_cast<const char *>(pats), n_pats * sizeof(Pattern));
    if (rows) key.append(reinterpret_cast<const char *>(rows->data()), rows->size());
    return pattern_get(dev, std::move(key), s, entry);
}

// What a launch path hands enqueue_launch: the plan its planner made (cec_launchplan.hpp)
// and what the sequence around the dispatch needs.
struct Launch {
    LaunchPlan plan;
    bool counted = true;  // by the fail hook (not the region multiply, nor the pool's flush)
    Tables tb{};          // the kernel's patterns (n_pats == 0: it has none); d == NULL: pinned
                          // here for the length of the enqueue, with `rows` behind them
    const std::vector<uint8_t> *rows = nullptr;
    const uint8_t *const *bases = nullptr;  // the argument block's streams, for the layout check
                                            // (NULL: the kernel's patterns name none by slot)
    int en = 0, el = 0;                     // the exact shape, for the refusal's message
    Tracker *uses[2] = {nullptr, nullptr};  // whose destroy waits for the launch's stream
};

static int plan_refused(const Launch &l) {
    const LaunchPlan &lp = l.plan;
    switch (lp.refusal) {
    case kPlanStreams:
        return fail(CEC_EINVAL, "internal: an op names more than %d byte streams; not launched", kMaxStreams);
    case kPlanLayout:
        return fail(CEC_EINVAL, "internal: a launch's argument block cannot serve its patterns "
                                "(kind %d, %d x %d); not launched", lp.kind, l.en, l.el);
    default:  // (the ops refuse these in their own words before they enqueue)
        return fail(CEC_EINVAL, "internal: kernel kind %d cannot run %llu tiles of %d x %d in one launch; not launched",
                    lp.kind, static_cast<unsigned long long>(lp.n_tiles), l.en, l.el);
    }
}

// The one enqueue sequence of the library, for every kernel with a launch record: the fail
// hook's countdown, the tables pinned, the layout check, `dispatch(plan, tables)` -- the
// path's own argument block and template dispatch --, the streams noted, the tables
// unpinned on every exit, hipGetLastError, the record.
template <class Dispatch>
static int enqueue_launch(int dev, hipStream_t stream, Launch &l, Dispatch &&dispatch) {
    if (l.counted)
        if (int r = launch_countdown()) return r;
    if (l.plan.refusal == kPlanNothing) return CEC_OK;
    PatEntry *entry = nullptr;
    if (l.plan.refusal == kPlanOk && l.tb.n_pats && !l.tb.d) {
        if (int r = pattern_tables(dev, l.tb.host, l.tb.n_pats, l.rows, stream, &entry)) return r;
        l.tb.d = entry->d;
    }
    if (l.bases) check_layout(l.plan, l.bases, l.tb);
    const int rc = l.plan.refusal == kPlanOk ? dispatch(l.plan, l.tb.d) : plan_refused(l);
    for (Tracker *u : l.uses)
        if (u) u->note(stream);  // (host-side only)
    if (entry) pattern_done(entry);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    record_launch(l.plan);
    return CEC_OK;
}

// One launch over the tiles of `src` with the patterns of `tb` (tb.d == NULL: pinned for the
// launch, with `rows`), recorded for cec_last_launch.
// *released: whether every wave of the launch ends with a system-scope release
// (kFlagSysRelease asked for, and honoured: only the narrow 1 x 1 launches carry it).
static int launch_combine(int dev, const Streams &st, const Tables &tb, const std::vector<uint8_t> *rows,
                          const LaunchShape &sh, bool lds, const TileSource &src, hipStream_t stream, bool counted,
                          uint32_t flags = 0, bool *released = nullptr) {
    uintptr_t bases_or = 0;
    for (int i = 0; i < kMaxStreams; ++i) bases_or |= reinterpret_cast<uintptr_t>(st.base[i]);
    Launch l;
    l.plan = plan_combine(sh, src.n_tiles, src.n_line_tiles, bases_or, lds, flags, g_knobs, waves_per_cu_cap(),
                          g_dev[dev].lds_per_cu);
    if (st.refused) l.plan.refusal = kPlanStreams;
    l.counted = counted;
    l.tb = tb;
    l.rows = rows;
    l.bases = st.base;
    l.en = sh.en;
    l.el = sh.el;
    l.uses[0] = src.uses;  // a plan's streams, for its destroy
    if (released) *released = l.plan.kind == kKindNarrow && (flags & kFlagSysRelease) != 0;
    return enqueue_launch(dev, stream, l, [&](const LaunchPlan &lp, const uint8_t *d) {
        CombineArgs a;
        memset(&a, 0, sizeof a);
        for (int i = 0; i < kMaxStreams; ++i) a.base[i] = st.base[i];
        a.tiles = src.tiles;
        a.implicit_len = src.implicit_len;
        a.patterns = reinterpret_cast<const Pattern *>(d);
        a.rows = d + tb.n_pats * sizeof(Pattern);
        a.n_tiles = static_cast<uint32_t>(lp.n_tiles);
        a.split_shift = lp.split_shift;
        a.grid = lp.grid;
        a.flags = lp.flags;
        a.wt_from = lp.wt_from;
        const bool perm = lp.engine == CEC_ENGINE_PERM;
        bool ok = true;
        if (lp.kind == kKindNarrow) {  // (the block the layout check saw: the first two slots)
            const CombineArgsN<kNarrowStreams> na = narrow_args(a);
            ok = perm ? launch_narrow<PermEngine>(na, lp, stream) : launch_narrow<LdsEngine>(na, lp, stream);
        } else if (lp.kind == kKindExact) {
            ok = perm ? launch_exact<PermEngine>(a, lp, stream) : launch_exact<LdsEngine>(a, lp, stream);
        } else {
            perm ? launch_generic<PermEngine>(a, lp, stream) : launch_generic<LdsEngine>(a, lp, stream);
        }
        return ok ? CEC_OK
                  : fail(CEC_EINVAL, "internal: no %s kernel for %d x %d", lp.kind == kKindNarrow ? "narrow" : "exact",
                         lp.nt, lp.lt);
    });
}

// One launch over a tile source with a pattern set built for `engine` (the patterns'
// coefficient form and the kernel must agree: the engine is read once per op, so a
// concurrent cec_set_engine cannot split them).  Counted by the fail hook even where the
// source is empty.
static int run_combine(int dev, const Streams &st, const std::vector<Pattern> &pats,
                       const std::vector<uint8_t> &rows, const TileSource &src, hipStream_t stream,
                       const std::vector<char> *used, int engine) {
    return launch_combine(dev, st, Tables{nullptr, pats.size(), pats.data(), used}, &rows,
                          src.n_tiles ? launch_shape(pats, used) : LaunchShape{}, engine == CEC_ENGINE_LDS, src, stream,
                          true);
}

// The patterns of launch g of a combo list: outputs [4g, 4g+4) of every combo, with the
// engine's coefficient form (and LDS rows).  The launches of one combo run in order on one
// stream, so no launch may read a stream an earlier launch of the combo wrote: an output
// that overwrites an input of its own combination is last in `outs` and runs in the final
// launch, after every group read the old bytes.  Two ops have one: the diff-update's install
// (the new value over the data shard) and cec_recovery_finish's R' (the new residual over
// the touched session's residual).
// This is where a Combo becomes a Pattern, so the Pattern's capacities are enforced here
// for every caller: at most kPatN inputs, and -- for a caller that launches group g alone
// (`only_group`: the region multiply, the pool's flush) -- no output past that group, which
// would be dropped unsaid.  Nothing is appended on a refusal.
static int build_patterns(const std::vector<Combo> &combos, size_t g, int engine, std::vector<Pattern> &pats,
                          std::vector<uint8_t> &rows, bool only_group = false) {
    for (const Combo &c : combos) {
        if (c.n_in < 0 || c.n_in > kPatN)
            return fail(CEC_EINVAL, "internal: a combination of %d inputs (a pattern holds %d); not launched",
                        c.n_in, kPatN);
        if (only_group && c.outs.size() > (g + 1) * kPatL)
            return fail(CEC_EINVAL, "internal: a combination of %zu outputs in one launch (a pattern holds %d); "
                                    "not launched", c.outs.size(), kPatL);
    }
    pats.reserve(pats.size() + combos.size());
    for (const Combo &c : combos) {
        Pattern p = blank_pattern();
        p.n_in = c.n_in;
        for (int i = 0; i < c.n_in; ++i) {
            p.in_stream[i] = c.in_stream[i];
            p.in_src[i] = c.in_src[i];
        }
        const size_t n = c.outs.size();
        const size_t lo = g * kPatL, hi = std::min(n, lo + kPatL);
        int no = 0;
        for (size_t o = lo; o < hi; ++o, ++no) {
            const Combo::Out &q = c.outs[o];
            p.out_stream[no] = q.stream;
            p.out_src[no] = q.src;
            p.out_mode[no] = q.mode;
            for (int i = 0; i < c.n_in; ++i) set_coef(p, no, i, q.coef[i], engine);
        }
        p.n_out = no;
        if (engine == CEC_ENGINE_LDS) assign_rows(p, rows);
        pats.push_back(p);
    }
    return CEC_OK;
}

// `used`: which combos the launch's tiles name (NULL = all; a persistent pattern table
// may hold more than one launch uses: the kernel shape is chosen from the used ones).
// `lds_op`: the op AUTO runs with the LDS engine (op_engine).
static int run_combos(int dev, const Streams &st, const std::vector<Combo> &combos, const TileSource &src,
                      hipStream_t stream, const std::vector<char> *used = nullptr, bool lds_op = false) {
    size_t max_out = 0;
    for (const Combo &c : combos) max_out = std::max(max_out, c.outs.size());
    const int engine = op_engine(lds_op);
    const size_t groups = (max_out + kPatL - 1) / kPatL;
    for (size_t g = 0; g < groups; ++g) {
        std::vector<Pattern> pats;
        std::vector<uint8_t> rows;
        if (int r = build_patterns(combos, g, engine, pats, rows)) return r;
        if (int r = run_combine(dev, st, pats, rows, src, stream, used, engine)) return r;
    }
    return CEC_OK;
}
// The ops' two forms: over the tiles of a plan, and over the region [0, len).
static int run_combos_plan(int dev, const Streams &st, const std::vector<Combo> &combos, const cec_plan *plan,
                           hipStream_t stream, bool lds_op = false) {
    TileSource src;
    if (int r = TileSource::of_plan(plan, dev, &src)) return r;
    return run_combos(dev, st, combos, src, stream, nullptr, lds_op);
}
static int run_combos_region(int dev, const Streams &st, const std::vector<Combo> &combos, uint64_t len,
                             hipStream_t stream) {
    TileSource src;
    if (int r = TileSource::of_region(len, &src)) return r;
    return run_combos(dev, st, combos, src, stream);
}

static int check_code(int k, int m, const int *matrix) {
    if (k < 1 || k > CEC_MAX_K || m < 1 || m > CEC_MAX_M || k + m > 32)
        return fail(CEC_EINVAL, "unsupported code k=%d m=%d (1<=k<=%d, 1<=m<=%d, k+m<=32)", k, m,
                    CEC_MAX_K, CEC_MAX_M);
    if (!matrix) return fail(CEC_EINVAL, "matrix is NULL");
    for (int i = 0; i < (k + m) * k; ++i)
        if (matrix[i] < 0 || matrix[i] > 255)
            return fail(CEC_EINVAL, "matrix entry %d = %d outside GF(2^8)", i, matrix[i]);
    return CEC_OK;
}

// ============================================================== arena layout
CEC_API size_t cec_arena_stride(size_t bytes) {
    size_t pages = (bytes + kTile - 1) / kTile;
    if (pages % 2 == 0) ++pages;  // odd number of 4 KiB pages between arena bases
    return pages * kTile;
}

CEC_API int cec_arenas_alloc(int count, size_t bytes, uint8_t **arenas, void **slab) {
    if (count < 1 || !arenas || !slab) return fail(CEC_EINVAL, "cec_arenas_alloc: bad args");
    *slab = nullptr;
    int dev;
    if (int r = current_device(&dev)) return r;
    const size_t stride = cec_arena_stride(bytes);
    uint8_t *base = nullptr;
    if (hipMalloc(&base, stride * static_cast<size_t>(count)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CEC_ENOMEM, "cec_arenas_alloc: %d x %zu bytes", count, stride);
    }
    for (int i = 0; i < count; ++i) arenas[i] = base + static_cast<size_t>(i) * stride;
    *slab = base;
    return CEC_OK;
}

CEC_API int cec_arenas_free(void *slab) {
    if (slab) HIP_TRY(hipFree(slab));
    return CEC_OK;
}

// ============================================================== runtime API
CEC_API const char *cec_version(void) { return "cocytus_ec 0.1 (gfx950)"; }
CEC_API const char *cec_last_error(void) { return g_err; }
CEC_API int cec_device_check(void) {
    int dev;
    return current_device(&dev);
}
CEC_API int cec_set_engine(cec_engine e) {
    if (e != CEC_ENGINE_PERM && e != CEC_ENGINE_LDS && e != CEC_ENGINE_AUTO)
        return fail(CEC_EINVAL, "bad engine %d", e);
    g_engine.store(e);
    return CEC_OK;
}
CEC_API cec_engine cec_get_engine(void) { return static_cast<cec_engine>(g_engine.load()); }
CEC_API int cec_last_engine(void) { return t_last_engine; }

// Test hook: the launch-time check (stream_layout_ok) on one pattern, as enqueue_launch
// runs it, for a narrow or a full argument block built from `bases`.  Host only.
CEC_API int cec_internal_check_launch_layout(int narrow, const int *in_slots, int n_in, const int *out_slots,
                                             int n_out, const void *const *bases, int n_bases) {
    if (n_in < 0 || n_in > kPatN || n_out < 0 || n_out > kPatL || n_bases < 0 || n_bases > kMaxStreams ||
        (n_in && !in_slots) || (n_out && !out_slots) || (n_bases && !bases))
        return fail(CEC_EINVAL, "cec_internal_check_launch_layout: bad args");
    Pattern p = blank_pattern();
    p.n_in = n_in;
    p.n_out = n_out;
    for (int i = 0; i < n_in; ++i) {
        if (in_slots[i] < 0 || in_slots[i] >= kMaxStreams) return fail(CEC_EINVAL, "slot %d", in_slots[i]);
        p.in_stream[i] = static_cast<uint8_t>(in_slots[i]);
    }
    for (int l = 0; l < n_out; ++l) {
        if (out_slots[l] < 0 || out_slots[l] >= kMaxStreams) return fail(CEC_EINVAL, "slot %d", out_slots[l]);
        p.out_stream[l] = static_cast<uint8_t>(out_slots[l]);
    }
    const uint8_t *block[kMaxStreams] = {};  // (a narrow block is the first two slots)
    for (int i = 0; i < n_bases; ++i) block[i] = static_cast<const uint8_t *>(bases[i]);
    if (!stream_layout_ok(block, narrow ? kNarrowStreams : kMaxStreams, Tables{nullptr, 1, &p, nullptr}))
        return fail(CEC_EINVAL, "internal: a launch's argument block cannot serve its patterns; not launched");
    return CEC_OK;
}
CEC_API int cec_set_waves_per_cu(int waves_per_cu) {
    if (waves_per_cu < 0 || waves_per_cu > 64) return fail(CEC_EINVAL, "bad waves_per_cu %d", waves_per_cu);
    g_waves_per_cu.store(waves_per_cu);
    return CEC_OK;
}
CEC_API int cec_get_waves_per_cu(void) { return waves_per_cu_cap(); }

// ============================================================== ops
// Region multiply (one input, one output, an implicit region) without the generic path:
// the tables of a thread's last (device, multby, add, engine) stay pinned in the cache
// and memoised, so a call skips building, copying and hashing its 1.7 KiB pattern and
// the lookup (tools/dropin_breakdown.hip: 3.4 us of host time per call against 0.9 us
// for an empty launch).  The memo is used only once the tables' upload is known
// complete (until then the cache orders each launch after it), and never while
// capturing (the cache then marks the tables: a launch inside a capture fills a
// RegionMemo of its own on the stack, which unpins them when the call returns).
namespace {
struct RegionMemo {
    int dev = -1, key = -1;
    PatEntry *e = nullptr;  // pinned while memoised
    LaunchShape shape;
    Pattern pat;            // the host copy (the launch's stream check)
    ~RegionMemo() {
        if (e) pattern_done(e);
    }
};
thread_local RegionMemo t_region;
}  // namespace

// `plain`: s is known not to be capturing (the drop-in's private stream).
// flags / *released: see launch_combine (the 1 x 1 region launches honour the release).
static int region_launch(int dev, const void *src, int multby, size_t n, void *dst, int add, hipStream_t s,
                         bool plain, uint32_t flags = 0, bool *released = nullptr) {
    TileSource region;
    if (int r = TileSource::of_region(n, &region)) return r;
    const int engine = op_engine(false);
    const int key = (engine << 9) | (add ? 256 : 0) | multby;
    const bool capturing = !plain && stream_capturing(s);
    Streams st;
    const int s_src = st.add(src), s_dst = st.add(dst);
    RegionMemo once;            // while capturing: tables pinned for this launch only
    RegionMemo *m = &t_region;  // the tables this launch runs with
    if (!(m->e && m->dev == dev && m->key == key && !capturing && m->e->up_done.load(std::memory_order_acquire))) {
        std::vector<Pattern> pats;
        std::vector<uint8_t> rows;
        if (int r = build_patterns({multiply_combo(multby, add, s_src, s_dst)}, 0, engine, pats, rows, true)) return r;
        PatEntry *e = nullptr;
        if (int r = pattern_tables(dev, pats.data(), pats.size(), &rows, s, &e)) return r;
        if (capturing) m = &once;           // (the cache marked the tables captured)
        else if (m->e) pattern_done(m->e);  // this launch's pin becomes the memo's
        m->dev = dev;
        m->key = key;
        m->e = e;
        m->shape = launch_shape(pats, nullptr);
        m->pat = pats[0];
    }
    return launch_combine(dev, st, Tables{m->e->d, 1, &m->pat, nullptr}, nullptr, m->shape, engine == CEC_ENGINE_LDS,
                          region, s, false, flags, released);
}

CEC_API int cec_region_multiply(const void *src, int multby, size_t nbytes, void *dst, int add,
                                void *stream) {
    if (!src || multby < 0 || multby > 255) return fail(CEC_EINVAL, "cec_region_multiply: bad args");
    int dev;
    if (int r = current_device(&dev)) return r;
    if (nbytes == 0) return CEC_OK;
    if (!dst) {
        dst = const_cast<void *>(src);
        add = 0;
    }
    if (add && multby == 0) return CEC_OK;
    return region_launch(dev, src, multby, nbytes, dst, add, static_cast<hipStream_t>(stream), false);
}

// AUTO's value-size rule for the decode: values of 64 KiB and more run the LDS engine,
// smaller ones (with erasures varying per value) PERM.  Measured on two boxes, two rounds
// each (profiles/r03_evidence/engine_auto/workloads_box*/; a third box agreed): at 64 KiB,
// 1 MiB and the mixed 256 B - 1 MiB batch the LDS engine led the rotating decode by
// 2.5-3.7 %, at 4 KiB PERM led it by 2-3 %.  The encode is within +-2 % at every size
// (LDS ahead by 0-1.6 % on large values, a tie at 4 KiB), so it runs PERM throughout.
static bool large_values(const cec_plan *plan) {
    return !plan || plan->total >= (uint64_t(64) << 10) * static_cast<uint64_t>(std::max(plan->n_ext, 1));
}

// The full-stripe encode as a combination, stated once for cec_encode / cec_encode_region and
// their digest-emitting forms: the k data arenas in, every live parity out.
struct EncodeCombo {
    Streams st;
    Combo c;
    int s_data[CEC_MAX_K], s_parity[CEC_MAX_M];  // the slot of each lid's arena
};
static int encode_combo(const char *op, const Code &code, const uint8_t *const *data, uint8_t *const *parity,
                        EncodeCombo *out) {
    for (int j = 0; j < code.k; ++j) {
        if (!data[j]) return fail(CEC_EINVAL, "%s: data[%d] is NULL", op, j);
        out->c.in(out->s_data[j] = out->st.add(data[j]));
    }
    for (int p = 0; p < code.m; ++p) {
        const int slot = out->s_parity[p] = out->st.add(parity[p]);
        if (!parity[p]) continue;  // a lost parity is simply not produced
        Combo::Out &o = out->c.out(slot, kModeWrite);
        for (int j = 0; j < code.k; ++j) o.coef[j] = code.at(code.k + p, j);
    }
    return CEC_OK;
}

static int encode_common(int k, int m, const int *matrix, const uint8_t *const *data,
                         uint8_t *const *parity, const cec_plan *plan, uint64_t len,
                         void *stream) {
    if (int r = check_code(k, m, matrix)) return r;
    if (!data || !parity) return fail(CEC_EINVAL, "cec_encode: NULL arena array");
    int dev;
    if (int r = current_device(&dev)) return r;
    EncodeCombo e;
    if (int r = encode_combo("cec_encode", Code{k, m, matrix}, data, parity, &e)) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return plan ? run_combos_plan(dev, e.st, {e.c}, plan, s) : run_combos_region(dev, e.st, {e.c}, len, s);
}

// Ops with one pattern index every tile's pattern field into a one-entry table: it must be 0.
static int single_pattern_plan(const cec_plan *plan, const char *op) {
    if (plan->n_ext && plan->max_pattern != 0)
        return fail(CEC_EINVAL, "%s: extent pattern %u, must be 0 for this op", op, plan->max_pattern);
    return CEC_OK;
}

CEC_API int cec_encode(int k, int m, const int *matrix, const uint8_t *const *data,
                       uint8_t *const *parity, const cec_plan *plan, void *stream) {
    if (!plan) return fail(CEC_EINVAL, "cec_encode: plan is NULL");
    if (int r = single_pattern_plan(plan, "cec_encode")) return r;
    return encode_common(k, m, matrix, data, parity, plan, 0, stream);
}

CEC_API int cec_encode_region(int k, int m, const int *matrix, const uint8_t *const *data,
                              uint8_t *const *parity, size_t len, void *stream) {
    return encode_common(k, m, matrix, data, parity, nullptr, len, stream);
}

CEC_API int cec_diff_update(int k, int m, const int *matrix, uint8_t *const *data,
                            const uint8_t *staging, uint8_t *const *parity, int install,
                            const cec_plan *plan, void *stream) {
    if (int r = check_code(k, m, matrix)) return r;
    if (!plan || !data || !staging || !parity) return fail(CEC_EINVAL, "cec_diff_update: NULL arg");
    if (plan->overlap) return fail(CEC_EOVERLAP, "cec_diff_update: plan extents overlap");
    if (plan->n_ext && plan->max_pattern >= static_cast<uint32_t>(k))
        return fail(CEC_EINVAL, "cec_diff_update: an extent names source shard %u (k = %d)", plan->max_pattern, k);
    int dev;
    if (int r = current_device(&dev)) return r;
    const Code code{k, m, matrix};
    Streams st;
    int s_data[CEC_MAX_K], s_parity[CEC_MAX_M];
    for (int j = 0; j < k; ++j) {
        if (!data[j]) return fail(CEC_EINVAL, "cec_diff_update: data[%d] is NULL", j);
        s_data[j] = st.add(data[j]);
    }
    for (int p = 0; p < m; ++p) s_parity[p] = st.add(parity[p]);
    const int s_staging = st.add(staging);
    std::vector<Combo> combos(k);
    for (int j = 0; j < k; ++j) {
        Combo &c = combos[j];
        const int old = c.in(s_data[j]);          // old bytes, arena offset
        const int nu = c.in(s_staging, true);     // new value, staging offset
        for (int p = 0; p < m; ++p) {
            if (!parity[p]) continue;  // lost parity: skipped like memcached.c:2692-2694
            Combo::Out &o = c.out(s_parity[p], kModeXor);
            o.coef[old] = o.coef[nu] = code.at(k + p, j);
        }
        if (install) c.out(s_data[j], kModeWrite).coef[nu] = 1;
    }
    // AUTO: PERM.  The LDS engine's diff-update was within +-3 % of PERM either way over
    // the recorded boxes (median margin under 1 %; DESIGN.md §4 "Engine per op").
    return run_combos_plan(dev, st, combos, plan, static_cast<hipStream_t>(stream));
}

CEC_API int cec_set_diff(int k, const uint8_t *const *data, const uint8_t *staging, uint8_t *diff,
                         const cec_plan *plan, void *stream) {
    if (k < 1 || k > CEC_MAX_K || !plan || !data || !staging || !diff)
        return fail(CEC_EINVAL, "cec_set_diff: bad args");
    if (plan->n_ext && plan->max_pattern >= static_cast<uint32_t>(k))
        return fail(CEC_EINVAL, "cec_set_diff: an extent names source shard %u (k = %d)", plan->max_pattern, k);
    int dev;
    if (int r = current_device(&dev)) return r;
    Streams st;
    int s_data[CEC_MAX_K];
    for (int j = 0; j < k; ++j) {
        if (!data[j]) return fail(CEC_EINVAL, "cec_set_diff: data[%d] is NULL", j);
        s_data[j] = st.add(data[j]);
    }
    const int s_staging = st.add(staging), s_diff = st.add(diff);
    std::vector<Combo> combos(k);
    for (int j = 0; j < k; ++j) {
        Combo &c = combos[j];
        const int old = c.in(s_data[j]), nu = c.in(s_staging, true);
        Combo::Out &o = c.out(s_diff, kModeWrite, true);
        o.coef[old] = o.coef[nu] = 1;
    }
    return run_combos_plan(dev, st, combos, plan, static_cast<hipStream_t>(stream));
}

CEC_API int cec_apply_diffs(int k, int m, const int *matrix, int lid_self, const uint8_t *diffs,
                            uint8_t *parity, const cec_plan *plan, void *stream) {
    if (int r = check_code(k, m, matrix)) return r;
    if (lid_self < k || lid_self >= k + m || !diffs || !parity || !plan)
        return fail(CEC_EINVAL, "cec_apply_diffs: bad args (lid_self=%d)", lid_self);
    if (plan->overlap) return fail(CEC_EOVERLAP, "cec_apply_diffs: plan extents overlap");
    if (plan->n_ext && plan->max_pattern >= static_cast<uint32_t>(k))
        return fail(CEC_EINVAL, "cec_apply_diffs: an extent names source shard %u (k = %d)", plan->max_pattern, k);
    int dev;
    if (int r = current_device(&dev)) return r;
    const Fold f = fold(Code{k, m, matrix}, lid_self, diffs, parity);
    return run_combos_plan(dev, f.st, f.combos, plan, static_cast<hipStream_t>(stream));
}

CEC_API int cec_residual(int k, int m, const int *matrix, int lid_self, uint32_t mask,
                         const uint8_t *const *arenas, uint8_t *residual, const cec_plan *plan,
                         void *stream) {
    if (int r = check_code(k, m, matrix)) return r;
    if (lid_self < k || lid_self >= k + m || !arenas || !residual || !plan)
        return fail(CEC_EINVAL, "cec_residual: bad args");
    if (int r = single_pattern_plan(plan, "cec_residual")) return r;
    // the parity itself plus one input per data lid of the mask: a pattern holds kPatN
    const int n_data = __builtin_popcount(mask & ((1u << k) - 1u));  // (k <= CEC_MAX_K: check_code)
    if (1 + n_data > kPatN)
        return fail(CEC_EINVAL, "cec_residual: mask 0x%x names %d data lids; with the parity that is more "
                                "than the %d inputs of one combination", mask, n_data, kPatN);
    int dev;
    if (int r = current_device(&dev)) return r;
    if (!arenas[lid_self]) return fail(CEC_EINVAL, "cec_residual: own parity arena is NULL");
    for (int s = 0; s < k; ++s)
        if ((mask & (1u << s)) && !arenas[s]) return fail(CEC_EINVAL, "cec_residual: arena %d in mask is NULL", s);
    const Code code{k, m, matrix};
    // one slot per lid, empty unless the combination reads it, then the residual's
    Streams st;
    int s_lid[CEC_MAX_K + CEC_MAX_M];
    for (int lid = 0; lid < k + m; ++lid)
        s_lid[lid] = st.add(lid == lid_self || (lid < k && (mask & (1u << lid))) ? arenas[lid] : nullptr);
    Combo c;
    Combo::Out &o = c.out(st.add(residual), kModeWrite);
    o.coef[c.in(s_lid[lid_self])] = 1;  // first touch copies the parity unit (recovery.c:79-82)
    for (int s = 0; s < k; ++s)
        if (mask & (1u << s)) o.coef[c.in(s_lid[s])] = code.at(lid_self, s);  // recovery.c:91-93
    return run_combos_plan(dev, st, {c}, plan, static_cast<hipStream_t>(stream));
}

CEC_API int cec_solve(int k, int m, const int *matrix, uint32_t mask,
                      const uint8_t *const *residuals, uint8_t *const *out, const cec_plan *plan,
                      void *stream) {
    if (int r = check_code(k, m, matrix)) return r;
    if (!mask_ok(k, m, mask) || !residuals || !out || !plan)
        return fail(CEC_EINVAL, "cec_solve: bad args (mask=0x%x)", mask);
    if (int r = single_pattern_plan(plan, "cec_solve")) return r;
    int dev;
    if (int r = current_device(&dev)) return r;
    Loss ls;
    if (int r = Loss::of(Code{k, m, matrix}, mask, "cec_solve", &ls)) return r;
    if (ls.n == 0) return CEC_OK;
    Streams st;
    Combo c;
    for (int r = 0; r < ls.n; ++r) {
        if (!residuals[ls.pars[r]]) return fail(CEC_EINVAL, "cec_solve: residual %d NULL", ls.pars[r]);
        c.in(st.add(residuals[ls.pars[r]]));
    }
    for (int x = 0; x < ls.n; ++x) {
        if (!out[ls.lost[x]]) return fail(CEC_EINVAL, "cec_solve: out[%d] NULL", ls.lost[x]);
        Combo::Out &o = c.out(st.add(out[ls.lost[x]]), kModeWrite);
        for (int r = 0; r < ls.n; ++r) o.coef[r] = ls.at(x, r);  // memcached.c:7916-7922
    }
    return run_combos_plan(dev, st, {c}, plan, static_cast<hipStream_t>(stream));
}

// The decode as combinations, one per mask, stated once for cec_decode and cec_decode_digests:
// the k lids of the mask in, the data lids it loses out.
struct DecodeCombos {
    Streams st;
    std::vector<Combo> combos;
    int s_arena[CEC_MAX_K + CEC_MAX_M], s_out[CEC_MAX_K];  // the slot of each lid's arena / output
    uint32_t lost = 0;                                     // the data lids some mask loses
};
static int decode_combos(const char *op, const Code &code, const uint32_t *masks, int n_masks,
                         const uint8_t *const *arenas, uint8_t *const *out, DecodeCombos *d) {
    const int k = code.k, m = code.m;
    Streams &st = d->st;
    for (int lid = 0; lid < k + m; ++lid) d->s_arena[lid] = st.add(arenas[lid]);
    for (int j = 0; j < k; ++j) d->s_out[j] = st.add(out[j]);
    d->combos.assign(n_masks, Combo());
    for (int q = 0; q < n_masks; ++q) {
        const uint32_t mask = masks[q];
        Loss ls;
        if (int r = Loss::of(code, mask, op, &ls)) return r;
        Combo &c = d->combos[q];
        // inputs: the n participating parities, then the k-n surviving data shards
        for (int i = 0; i < k; ++i) {
            const int lid = i < ls.n ? ls.pars[i] : ls.surv[i - ls.n];
            if (!arenas[lid]) return fail(CEC_EINVAL, "%s: arena %d (in mask 0x%x) is NULL", op, lid, mask);
            c.in(d->s_arena[lid]);
        }
        // D_lost[x] = sum_r inv[x][r] * (P_r ^ sum_s M[P_r][s] * D_s)
        for (int x = 0; x < ls.n; ++x) {
            if (!out[ls.lost[x]]) return fail(CEC_EINVAL, "%s: out[%d] is NULL", op, ls.lost[x]);
            d->lost |= 1u << ls.lost[x];
            Combo::Out &o = c.out(d->s_out[ls.lost[x]], kModeWrite);
            for (int r = 0; r < ls.n; ++r) o.coef[r] = ls.at(x, r);
            for (int s = 0; s < ls.n_surv; ++s)
                for (int r = 0; r < ls.n; ++r) o.coef[ls.n + s] ^= gf_mul(ls.at(x, r), code.at(ls.pars[r], ls.surv[s]));
        }
    }
    return CEC_OK;
}

CEC_API int cec_decode(int k, int m, const int *matrix, const uint32_t *masks, int n_masks,
                       const uint8_t *const *arenas, uint8_t *const *out, const cec_plan *plan,
                       void *stream) {
    if (int r = check_code(k, m, matrix)) return r;
    if (!masks || n_masks < 1 || !arenas || !out || !plan)
        return fail(CEC_EINVAL, "cec_decode: bad args");
    int dev;
    if (int r = current_device(&dev)) return r;
    if (plan->n_ext && plan->max_pattern >= static_cast<uint32_t>(n_masks))
        return fail(CEC_EINVAL, "cec_decode: an extent names mask %u of %d", plan->max_pattern, n_masks);
    DecodeCombos d;
    if (int r = decode_combos("cec_decode", Code{k, m, matrix}, masks, n_masks, arenas, out, &d)) return r;
    // AUTO: values of 64 KiB and more (large_values) run the LDS engine, ahead of PERM by a
    // median 3 % there (rotating or one mask: configs[4]'s 1 MiB D1-by-P1 rebuild +4.9 %);
    // 4 KiB values run PERM (rotating masks -1.7 %, one mask +1.1 %: within 2 %)
    return run_combos_plan(dev, d.st, d.combos, plan, static_cast<hipStream_t>(stream), large_values(plan));
}

CEC_API uint32_t cec_recovery_mask(int k, int m, int leader_lid, const int *connected) {
    if (k < 1 || m < 1 || k + m > 32 || !connected || leader_lid < 0 || leader_lid >= k + m)
        return 0;
    int remaining = k - 1;
    uint32_t mask = 1u << leader_lid;
    for (int i = 0; i < k + m && remaining; ++i) {
        if (i == leader_lid || !connected[i]) continue;
        mask |= 1u << i;
        --remaining;
    }
    return remaining ? 0u : mask;
}

// ============================================================== fast stream wait
// One lane stores v into mapped pinned memory once every earlier op on the stream has
// finished (stream order).
__global__ void cec_signal_kernel(uint32_t *flag, uint32_t v) {
    __threadfence_system();
    __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

namespace {
struct SignalCtx {  // per thread and device: a mapped pinned completion word
    int device = -1;
    Buf flag;  // (idle when released: every wait completed before its call returned)
    uint32_t seq = 0;
    hipEvent_t fence = nullptr;  // recorded before the signal: a system-scope release
    ~SignalCtx() {
        if (fence) (void)hipEventDestroy(fence);
    }
};
thread_local SignalCtx t_signal;
}  // namespace

// Wait for everything enqueued on stream s, for the synchronous calls whose cost is
// their latency (the per-call drop-in, per-SET recovery folds).  A one-lane kernel
// writes a sequence number into mapped pinned memory behind the work and the host
// spins on it: 6.3 us per empty call against 10.5 us for hipStreamSynchronize
// (tools/launch_latency.hip, archive/profiles/r01_launch_latency.txt).  After 200 us (a large
// op, or a kernel that faulted and never signals) it falls back to
// hipStreamSynchronize, which also reports errors.
// `host_results`: the work wrote host-visible memory that the caller reads on return;
// `waves_released`: every wave that wrote it ended with its own system-scope release
// (kFlagSysRelease).  The completion is recorded for cec_last_sync.
thread_local cec_sync_record t_last_sync = {0, 0, 0, 0};

static int stream_wait(hipStream_t s, bool host_results, bool waves_released = false) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    SignalCtx &c = t_signal;
    if (c.device != dev) {
        c.device = -1;
        if (!c.flag.acquire_mapped(dev, 64)) return fail(CEC_ENOMEM, "completion flag");
        __atomic_store_n(c.flag.get<uint32_t>(), 0u, __ATOMIC_RELEASE);
        c.seq = 0;
        if (c.fence) (void)hipEventDestroy(c.fence);
        c.fence = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&c.fence, hipEventDisableTiming));
        c.device = dev;
    }
    const uint32_t v = ++c.seq;
    const bool fence = host_results && !waves_released;
    t_last_sync.seq += 1;
    t_last_sync.host_results = host_results;
    t_last_sync.waves_released = host_results && waves_released;
    t_last_sync.fenced = fence;
    // The op's stores into host memory may still sit in the L2 of the XCDs its
    // workgroups ran on, and the signal kernel's own fence writes back only its XCD's
    // (a 4098-byte drop-in call read back its second tile stale on some boxes).  Either
    // every wave of the op ended with a system-scope release (kFlagSysRelease: the
    // drop-in), or an event recorded here with the system fence makes the command
    // processor write every L2 back before the signal kernel starts (4-5 us more per
    // call on one box, archive/profiles/r02_evidence_s3/fence_cost_ab.jsonl).  (Spinning on
    // hipEventQuery of that event instead of the signal kernel's flag measured the same
    // per call: archive/profiles/r02_evidence_s3/wait_mode_ab.jsonl.)
    if (fence) HIP_TRY(hipEventRecord(c.fence, s));
    hipLaunchKernelGGL(cec_signal_kernel, dim3(1), dim3(1), 0, s, c.flag.alias<uint32_t>(), v);
    HIP_TRY(hipGetLastError());
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t *flag = c.flag.get<uint32_t>();
    for (uint32_t i = 1;; ++i) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == v) return CEC_OK;
        __builtin_ia32_pause();
        if ((i & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200))
            break;
    }
    HIP_TRY(hipStreamSynchronize(s));
    return CEC_OK;
}

CEC_API int cec_last_sync(cec_sync_record *out) {
    if (!out) return fail(CEC_EINVAL, "cec_last_sync: out is NULL");
    *out = t_last_sync;
    return CEC_OK;
}

#include "cec_drain.inc"
#include "cec_recovery.inc"
#include "cec_pool.inc"
#include "cec_hostbatch.inc"
#include "cec_scrub.inc"
#include "cec_digest.inc"

// ============================================================== events / streams
CEC_API int cec_event_create(void **ev) {
    if (!ev) return fail(CEC_EINVAL, "NULL");
    hipEvent_t e;
    // Timing events only: no system-scope fence at record (the default fence writes the
    // L2 back between launches, which lengthens the measured interval).
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    *ev = e;
    return CEC_OK;
}
CEC_API int cec_event_destroy(void *ev) {
    HIP_TRY(hipEventDestroy(static_cast<hipEvent_t>(ev)));
    return CEC_OK;
}
CEC_API int cec_event_record(void *ev, void *stream) {
    HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(ev), static_cast<hipStream_t>(stream)));
    return CEC_OK;
}
CEC_API int cec_event_elapsed_ms(void *a, void *b, float *ms) {
    HIP_TRY(hipEventSynchronize(static_cast<hipEvent_t>(b)));
    HIP_TRY(hipEventElapsedTime(ms, static_cast<hipEvent_t>(a), static_cast<hipEvent_t>(b)));
    return CEC_OK;
}
CEC_API int cec_stream_synchronize(void *stream) {
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return CEC_OK;
}
CEC_API int cec_device_count(int *count) {
    if (!count) return fail(CEC_EINVAL, "cec_device_count: NULL");
    *count = 0;
    if (hipGetDeviceCount(count) != hipSuccess) {
        (void)hipGetLastError();
        *count = 0;
    }
    return CEC_OK;
}
CEC_API int cec_set_device(int device) {
    HIP_TRY(hipSetDevice(device));
    int dev;
    return current_device(&dev);
}
CEC_API int cec_stream_create(void **stream) {
    if (!stream) return fail(CEC_EINVAL, "cec_stream_create: NULL");
    hipStream_t s;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return CEC_OK;
}
CEC_API int cec_stream_destroy(void *stream) {
    HIP_TRY(hipStreamDestroy(static_cast<hipStream_t>(stream)));
    return CEC_OK;
}
CEC_API int cec_copy(void *dst, const void *src, size_t n, void *stream) {
    if (n && (!dst || !src)) return fail(CEC_EINVAL, "cec_copy: NULL pointer");
    int dev;
    if (int r = current_device(&dev)) return r;
    if (n) HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDefault, static_cast<hipStream_t>(stream)));
    return CEC_OK;
}

CEC_API int cec_host_register(void *p, size_t bytes, uint8_t **device_alias) {
    if (!p || !bytes || !device_alias) return fail(CEC_EINVAL, "cec_host_register: bad args");
    *device_alias = nullptr;
    int dev;
    if (int r = current_device(&dev)) return r;
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterMapped));
    void *d = nullptr;
    if (hipError_t e = hipHostGetDevicePointer(&d, p, 0); e != hipSuccess) {
        (void)hipHostUnregister(p);
        return fail(CEC_EHIP, "cec_host_register: hipHostGetDevicePointer: %s", hipGetErrorString(e));
    }
    *device_alias = static_cast<uint8_t *>(d);
    host_region_add(p, bytes, *device_alias, dev);  // (the host batch reads bases there in place)
    return CEC_OK;
}

CEC_API int cec_host_unregister(void *p) {
    if (!p) return fail(CEC_EINVAL, "cec_host_unregister: NULL");
    int dev;
    if (int r = current_device(&dev)) return r;
    host_region_remove(p);
    HIP_TRY(hipHostUnregister(p));
    return CEC_OK;
}

// ============================================================== Jerasure drop-in
CEC_API int galois_single_multiply(int a, int b, int w) {
    if (w != 8) die("galois_single_multiply: only w = 8 is provided");
    return gf_mul(a, b);
}
CEC_API int galois_single_divide(int a, int b, int w) {
    if (w != 8) die("galois_single_divide: only w = 8 is provided");
    if ((b & 0xFF) == 0) return -1;
    return gf_div(a, b);
}
CEC_API int galois_inverse(int x, int w) { return galois_single_divide(1, x, w); }

CEC_API int *reed_sol_extended_vandermonde_matrix(int rows, int cols, int w) {
    if (w != 8 || rows < 1 || cols < 1 || rows > 256 || cols > 256) return nullptr;
    int *v = static_cast<int *>(calloc(static_cast<size_t>(rows) * cols, sizeof(int)));
    if (!v) return nullptr;
    v[0] = 1;
    if (rows == 1) return v;
    v[rows * cols - 1] = 1;
    for (int r = 1; r + 1 < rows; ++r)
        for (int c = 0, x = 1; c < cols; ++c, x = gf_mul(x, r)) v[r * cols + c] = x;
    return v;
}

CEC_API int *reed_sol_big_vandermonde_distribution_matrix(int rows, int cols, int w) {
    if (cols >= rows) return nullptr;
    int *m = reed_sol_extended_vandermonde_matrix(rows, cols, w);
    if (!m) return nullptr;
    auto at = [&](int r, int c) -> int & { return m[r * cols + c]; };
    for (int i = 1; i < cols; ++i) {  // column-reduce the top block to identity
        int r = i;
        while (r < rows && at(r, i) == 0) ++r;
        if (r == rows) { free(m); return nullptr; }
        if (r != i)
            for (int c = 0; c < cols; ++c) std::swap(at(r, c), at(i, c));
        if (at(i, i) != 1) {
            const int s = gf_inv(at(i, i));
            for (int q = 0; q < rows; ++q) at(q, i) = gf_mul(s, at(q, i));
        }
        for (int c = 0; c < cols; ++c) {
            const int e = at(i, c);
            if (c != i && e)
                for (int q = 0; q < rows; ++q) at(q, c) ^= gf_mul(e, at(q, i));
        }
    }
    for (int c = 0; c < cols; ++c) {  // first parity row -> all ones
        const int e = at(cols, c);
        if (e != 1) {
            const int s = gf_inv(e);
            for (int q = cols; q < rows; ++q) at(q, c) = gf_mul(s, at(q, c));
        }
    }
    for (int q = cols + 1; q < rows; ++q) {  // first column of later parity rows -> one
        const int e = at(q, 0);
        if (e != 1) {
            const int s = gf_inv(e);
            for (int c = 0; c < cols; ++c) at(q, c) = gf_mul(at(q, c), s);
        }
    }
    return m;
}

CEC_API int jerasure_invert_matrix(int *mat, int *inv, int rows, int w) {
    if (w != 8) {
        fprintf(stderr, "libcocytus_ec: jerasure_invert_matrix: only w = 8 is provided\n");
        return -1;
    }
    if (!mat || !inv || rows < 1) return -1;
    return invert_matrix(mat, inv, rows);
}

CEC_API int *jerasure_matrix_multiply(int *m1, int *m2, int r1, int c1, int r2, int c2, int w) {
    if (w != 8 || c1 != r2 || r1 < 1 || c2 < 1) return nullptr;
    int *p = static_cast<int *>(calloc(static_cast<size_t>(r1) * c2, sizeof(int)));
    if (!p) return nullptr;
    for (int i = 0; i < r1; ++i)
        for (int j = 0; j < c2; ++j) {
            int acc = 0;
            for (int x = 0; x < c1; ++x) acc ^= gf_mul(m1[i * c1 + x], m2[x * c2 + j]);
            p[i * c2 + j] = acc;
        }
    return p;
}

// Per-thread context of the synchronous drop-in: a stream and device staging.
namespace {
struct DropInCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    Buf dsrc, ddst;  // device staging of the chunked path
    Buf zc;  // mapped pinned buffer (2 x zc_cap) for zero-copy calls
    size_t zc_cap = 0;
    ~DropInCtx() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        release();
    }
    // Buffers back to the process caches (idle: every call completed before returning);
    // freeing them would wait for the whole device.
    void release() {
        dsrc.release();
        ddst.release();
        zc.release();
        zc_cap = 0;
    }
};
thread_local DropInCtx t_ctx;
constexpr size_t kStageChunk = size_t(64) << 20;

// Pageable calls up to this size go zero-copy: the bytes are memcpy'd into a mapped
// pinned buffer and the kernel reads / writes it over PCIe, which saves the three DMA
// set-ups of the staged path (latency-bound at 4 KiB).  CEC_DROPIN_ZC_MAX overrides.
size_t zero_copy_max() {
    static const size_t v = [] {
        const char *e = getenv("CEC_DROPIN_ZC_MAX");
        return e ? static_cast<size_t>(strtoull(e, nullptr, 0)) : size_t(256) << 10;
    }();
    return v;
}

}  // namespace

#define DROPIN_CHECK(expr)                                                                  \
    do {                                                                                    \
        int rc_ = (expr);                                                                   \
        if (rc_ != CEC_OK) {                                                                \
            char b_[640];                                                                   \
            snprintf(b_, sizeof b_, "galois_w08_region_multiply: %s", g_err);              \
            die(b_);                                                                        \
        }                                                                                   \
    } while (0)
#define DROPIN_HIP(expr)                                                                    \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            char b_[256];                                                                   \
            snprintf(b_, sizeof b_, "galois_w08_region_multiply: %s: %s", #expr,           \
                     hipGetErrorString(e_));                                                \
            die(b_);                                                                        \
        }                                                                                   \
    } while (0)

CEC_API void galois_w08_region_multiply(char *region, int multby, int nbytes, char *r2, int add) {
    if (multby < 0 || multby > 255) die("galois_w08_region_multiply: multby outside [0, 255]");
    if (nbytes <= 0) return;
    if (!region) die("galois_w08_region_multiply: region is NULL");
    if (r2 && add && multby == 0) return;
    int dev;
    DROPIN_CHECK(current_device(&dev));
    DropInCtx &c = t_ctx;
    if (c.device != dev) {
        if (c.stream) DROPIN_HIP(hipStreamDestroy(c.stream));
        c.stream = nullptr;
        c.release();  // (device addresses of the mapped buffer are per device)
        DROPIN_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        c.device = dev;
    }
    const size_t n = static_cast<size_t>(nbytes);
    char *dst = r2 ? r2 : region;
    const int mode_add = r2 ? add : 0;
    const PtrKind ks = classify(region), kd = classify(dst);
    void *const vs = ks.dev, *const vd = kd.dev;
    const bool hs = ks.host, hd = kd.host;
    if (vs && vd) {  // device-resident (or pinned/mapped): run in place
        bool rel = false;  // (a host-visible destination: the kernel's waves release it themselves)
        DROPIN_CHECK(region_launch(dev, vs, multby, n, vd, mode_add, c.stream, true, hd ? kFlagSysRelease : 0, &rel));
        DROPIN_CHECK(stream_wait(c.stream, hd, rel));
        return;
    }
    const size_t n16 = (n + 15) & ~size_t(15);  // the kernel's extent in the staging
    const bool host_ok = (!vs || hs) && (!vd || hd);  // both reachable by the CPU's memcpy
    if (host_ok && n <= zero_copy_max()) {  // small host call: zero-copy through mapped pinned memory
        if (c.zc_cap < n16) {
            c.zc_cap = std::max(n16, size_t(64) << 10);
            if (!c.zc.acquire_mapped(dev, 2 * c.zc_cap)) die("galois_w08_region_multiply: mapped staging allocation failed");
        }
        uint8_t *zs = c.zc.get(), *zd = zs + c.zc_cap;
        memcpy(zs, region, n);
        if (mode_add) memcpy(zd, dst, n);
        uint8_t *ds = c.zc.alias(), *dd = ds + c.zc_cap;
        // n16 bytes: whole 16-byte chunks only, no byte scatter over PCIe (the padding's
        // results are not copied back)
        bool rel = false;
        DROPIN_CHECK(region_launch(dev, ds, multby, n16, dd, mode_add, c.stream, true, kFlagSysRelease, &rel));
        DROPIN_CHECK(stream_wait(c.stream, true, rel));  // (spinning on hipStreamQuery instead: no gain)
        memcpy(dst, zd, n);
        return;
    }
    // larger host buffers (or a device operand with a host result): stage through
    // device memory chunk by chunk
    const size_t want = std::min(n, kStageChunk);
    if (c.ddst.bytes() < want &&
        (!c.dsrc.acquire(dev_cache(), dev, want) || !c.ddst.acquire(dev_cache(), dev, want)))
        die("galois_w08_region_multiply: device staging allocation failed");
    uint8_t *const dsrc = c.dsrc.get(), *const ddst = c.ddst.get();
    for (size_t o = 0; o < n; o += kStageChunk) {
        const size_t len = std::min(kStageChunk, n - o);
        DROPIN_HIP(hipMemcpyAsync(dsrc, region + o, len, hipMemcpyDefault, c.stream));
        if (mode_add)
            DROPIN_HIP(hipMemcpyAsync(ddst, dst + o, len, hipMemcpyDefault, c.stream));
        DROPIN_CHECK(region_launch(dev, dsrc, multby, len, ddst, mode_add, c.stream, true));
        DROPIN_HIP(hipMemcpyAsync(dst + o, ddst, len, hipMemcpyDefault, c.stream));
        DROPIN_HIP(hipStreamSynchronize(c.stream));
    }
    // (the result came back by DMA, complete and visible when the stream synchronised)
    t_last_sync.seq += 1;
    t_last_sync.host_results = !vd || hd;
    t_last_sync.waves_released = 0;
    t_last_sync.fenced = 1;
}
