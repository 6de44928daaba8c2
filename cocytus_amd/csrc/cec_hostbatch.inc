// cec_hostbatch.inc -- galois_w08_region_multiply, batched, over host memory.
// Included by cec_runtime.hip after cec_recovery.inc (shares PackPool, stream_wait and
// the launch internals); not a separate TU.
//
// The unchanged server keeps its recovery state in host memory: one malloc'd 4 KiB
// buffer per recovery unit (recovery.c:79), the parity arena `ecmem` (recovery.c:81),
// malloc'd peer replies and diffs (memcached.c:4321-4322), calloc'd solve outputs
// (memcached.c:7913).  It calls galois_w08_region_multiply once per unit
// (recovery.c:91, 123; memcached.c:7918).  cec_region_multiply_batch takes a whole list
// of those calls and runs them as ONE pass of the combine kernel per overlap wave:
//
//   pieces    each job is cut into pieces of <= kHbPiece bytes (pieces of one job are
//             independent byte ranges);
//   clusters  pieces whose dst ranges overlap form a cluster; a cluster is staged once,
//             so every piece that writes a byte writes the same staged byte;
//   waves     within a cluster, pieces that overlap run in separate launches: in job
//             order when a cluster holds a write (order matters), else by greedy
//             colouring (XOR accumulation commutes);
//   staging   one mapped pinned area per thread: [D: clusters][S: sources][B: bases];
//             the pack pool copies the caller's bytes in, the kernel reads and writes
//             the area over PCIe (zero-copy: no DMA set-up per call), the pool copies the
//             clusters back out;
//   tiles     off = the piece's byte in D, src_off = its byte in S (and, at a fixed
//             distance, in B): the same Tile / Pattern machinery as every other op.
// A round holds as many clusters as the staging fits; larger batches take several.
//
// Patterns (one per distinct (kind, multby) of the batch):
//   XOR   D ^= c * S          galois_w08_region_multiply(src, c, len, dst, 1)
//   WRITE D  = c * S          ... add = 0
//   BASE  D  = B ^ c * S      first touch: memcpy(dst, base), then add = 1 (recovery.c:79-91)

namespace {

constexpr size_t kHbPiece = size_t(1) << 20;          // bytes per piece of a job
constexpr size_t kHbStage = size_t(24) << 20;         // default staging (grows for one cluster)
constexpr size_t kHbParallelCopy = size_t(1) << 20;   // copies below this stay on one thread
constexpr size_t kHbPipeMin = size_t(4) << 20;        // batches above this are pipelined ...
constexpr uint64_t kHbPipeRounds = 4;                 // ... over at least this many rounds

// Host regions registered through cec_host_register (the server's ecmem): a batch whose
// bases all lie in one of them reads the bases in place, through the region's device alias,
// instead of packing them (the first-touch parity units of a recovery, the old bytes of SET
// diffs).  Regions registered with hipHostRegister directly are not known here: staged.
struct HostRegion {
    uintptr_t lo = 0, hi = 0;
    uint8_t *alias = nullptr;
    int dev = -1;
};
std::mutex &host_regions_mu() {
    static std::mutex *m = new std::mutex;  // (never destroyed: used from the exit path too)
    return *m;
}
std::vector<HostRegion> &host_regions() {
    static std::vector<HostRegion> *v = new std::vector<HostRegion>;
    return *v;
}
void host_region_add(void *p, size_t n, uint8_t *alias, int dev) {
    std::lock_guard<std::mutex> lk(host_regions_mu());
    host_regions().push_back(HostRegion{reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + n, alias, dev});
}
void host_region_remove(void *p) {
    std::lock_guard<std::mutex> lk(host_regions_mu());
    auto &v = host_regions();
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i].lo == reinterpret_cast<uintptr_t>(p)) {
            v.erase(v.begin() + static_cast<long>(i));
            return;
        }
}
// The registered region of device dev holding [a, a + n), if any.
bool host_region_find(uintptr_t a, size_t n, int dev, HostRegion *out) {
    std::lock_guard<std::mutex> lk(host_regions_mu());
    for (const HostRegion &r : host_regions())
        if (r.dev == dev && a >= r.lo && a + n <= r.hi) {
            *out = r;
            return true;
        }
    return false;
}

enum HbKind : uint8_t { kHbXor = 0, kHbWrite = 1, kHbBase = 2 };

struct HbPiece {
    const uint8_t *src, *base;
    uint8_t *dst;
    uint32_t len;
    uint8_t kind, multby;
    int job;         // caller's job index (order)
    int cluster;
    int wave;
    int pat;
    uint64_t soff;   // byte offset in S (and B) of this round
};

struct HbCluster {
    uintptr_t lo, hi;
    int first, count;  // pieces [first, first + count) of the cluster-sorted order
    bool packed;       // dst bytes staged in (some byte is read before it is written)
    int waves;
    uint64_t doff;
};

// Range-assign / range-max tree over compressed coordinates: the wave of a piece of a
// cluster holding a write is 1 + the highest wave of the earlier pieces it overlaps.
class MaxTree {
  public:
    explicit MaxTree(size_t n) : n_(std::max<size_t>(n, 1)), mx_(4 * n_, -1), lz_(4 * n_, -2) {}
    int query(size_t l, size_t r) { return q(1, 0, n_, l, r); }
    void assign(size_t l, size_t r, int v) { a(1, 0, n_, l, r, v); }

  private:
    void push(size_t x) {
        if (lz_[x] == -2) return;
        for (size_t c : {2 * x, 2 * x + 1}) mx_[c] = lz_[c] = lz_[x];
        lz_[x] = -2;
    }
    int q(size_t x, size_t lo, size_t hi, size_t l, size_t r) {
        if (r <= lo || hi <= l) return -1;
        if (l <= lo && hi <= r) return mx_[x];
        push(x);
        const size_t mid = (lo + hi) / 2;
        return std::max(q(2 * x, lo, mid, l, r), q(2 * x + 1, mid, hi, l, r));
    }
    void a(size_t x, size_t lo, size_t hi, size_t l, size_t r, int v) {
        if (r <= lo || hi <= l) return;
        if (l <= lo && hi <= r) {
            mx_[x] = lz_[x] = v;
            return;
        }
        push(x);
        const size_t mid = (lo + hi) / 2;
        a(2 * x, lo, mid, l, r, v);
        a(2 * x + 1, mid, hi, l, r, v);
        mx_[x] = std::max(mx_[2 * x], mx_[2 * x + 1]);
    }
    size_t n_;
    std::vector<int> mx_, lz_;
};

// Waves of one cluster's pieces (ids = indices into pc, in cluster-sorted order).
// Returns the number of waves; sets packed (some byte is read before any write).
int hb_cluster_waves(std::vector<HbPiece> &pc, const int *ids, int count, bool *packed) {
    if (count == 1) {
        pc[ids[0]].wave = 0;
        *packed = pc[ids[0]].kind == kHbXor;
        return 1;
    }
    bool writes = false;
    for (int i = 0; i < count; ++i) writes |= pc[ids[i]].kind != kHbXor;
    *packed = true;  // (a multi-piece cluster: conservatively staged in)
    if (!writes) {
        // greedy colouring over start-sorted pieces (ids are sorted by dst start)
        std::vector<std::pair<uintptr_t, int>> open;  // (end, wave), min-heap on end
        std::vector<int> free_w;
        int nw = 0;
        auto cmp = [](const std::pair<uintptr_t, int> &a, const std::pair<uintptr_t, int> &b) {
            return a.first > b.first;
        };
        for (int i = 0; i < count; ++i) {
            HbPiece &p = pc[ids[i]];
            const uintptr_t lo = reinterpret_cast<uintptr_t>(p.dst);
            while (!open.empty() && open.front().first <= lo) {
                free_w.push_back(open.front().second);
                std::pop_heap(open.begin(), open.end(), cmp);
                open.pop_back();
            }
            int w;
            if (!free_w.empty()) {
                auto it = std::min_element(free_w.begin(), free_w.end());
                w = *it;
                free_w.erase(it);
            } else {
                w = nw++;
            }
            p.wave = w;
            open.emplace_back(lo + p.len, w);
            std::push_heap(open.begin(), open.end(), cmp);
        }
        return std::max(nw, 1);
    }
    // job order: wave = 1 + the highest wave among earlier overlapping pieces
    std::vector<uintptr_t> xs;
    xs.reserve(2 * count);
    for (int i = 0; i < count; ++i) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(pc[ids[i]].dst);
        xs.push_back(lo);
        xs.push_back(lo + pc[ids[i]].len);
    }
    std::sort(xs.begin(), xs.end());
    xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
    std::vector<int> ord(ids, ids + count);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return pc[a].job < pc[b].job; });
    MaxTree tree(xs.size());
    int nw = 0;
    for (int id : ord) {
        HbPiece &p = pc[id];
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p.dst);
        const size_t l = std::lower_bound(xs.begin(), xs.end(), lo) - xs.begin();
        const size_t r = std::lower_bound(xs.begin(), xs.end(), lo + p.len) - xs.begin();
        p.wave = tree.query(l, r) + 1;
        tree.assign(l, r, p.wave);
        nw = std::max(nw, p.wave + 1);
    }
    return nw;
}

// (key, index) pairs sorted by key: LSD radix sort, 11-bit digits, digits on which every
// key agrees skipped (host addresses of one batch differ in their low ~40 bits: <= 4 passes).
void hb_radix_sort(std::vector<std::pair<uint64_t, int>> &a) {
    if (a.size() < 1024) {  // (a radix pass touches 2,049 counters: small batches sort faster)
        std::sort(a.begin(), a.end());
        return;
    }
    uint64_t orv = 0, andv = ~0ull;
    for (const auto &x : a) {
        orv |= x.first;
        andv &= x.first;
    }
    const uint64_t varies = orv ^ andv;
    std::vector<std::pair<uint64_t, int>> b(a.size());
    for (int shift = 0; shift < 64; shift += 11) {
        if (((varies >> shift) & 0x7FF) == 0) continue;
        size_t cnt[2049] = {};
        for (const auto &x : a) ++cnt[((x.first >> shift) & 0x7FF) + 1];
        for (int d = 0; d < 2048; ++d) cnt[d + 1] += cnt[d];
        for (const auto &x : a) b[cnt[(x.first >> shift) & 0x7FF]++] = x;  // stable
        a.swap(b);
    }
}

struct HbCopy {
    uint8_t *dst;
    const uint8_t *src;
    size_t len;
};

// Copies through the pack pool: thread t takes bytes [t*B/T, (t+1)*B/T) of the list.
void hb_copy(PackPool *pool, const std::vector<HbCopy> &items) {
    size_t total = 0;
    for (const HbCopy &c : items) total += c.len;
    if (!pool || pool->size() == 1 || total < kHbParallelCopy) {
        for (const HbCopy &c : items) memcpy(c.dst, c.src, c.len);
        return;
    }
    std::vector<size_t> prefix(items.size() + 1, 0);
    for (size_t i = 0; i < items.size(); ++i) prefix[i + 1] = prefix[i] + items[i].len;
    const int T = pool->size();
    pool->run([&](int t) {
        const size_t lo = total * t / T, hi = total * (t + 1) / T;
        if (lo >= hi) return;
        size_t i = std::upper_bound(prefix.begin(), prefix.end(), lo) - prefix.begin() - 1;
        for (size_t pos = lo; pos < hi && i < items.size(); ++i) {
            const HbCopy &c = items[i];
            const size_t a = pos - prefix[i], b = std::min(c.len, hi - prefix[i]);
            if (b > a) memcpy(c.dst + a, c.src + a, b - a);
            pos = prefix[i] + b;
        }
    });
}

struct HostBatchCtx {  // per thread and device
    int device = -1;
    uint8_t *stage = nullptr;  // mapped pinned
    uint8_t *stage_dev = nullptr;
    size_t cap = 0;
    Tile *h_tiles = nullptr, *d_tiles = nullptr;
    size_t tile_cap = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};  // round completion per staging half (pipelined batches)
    std::unique_ptr<PackPool> pool;
    int last_launches = 0, last_rounds = 0, last_in_place = 0;
    double t_plan = 0, t_pack = 0, t_gpu = 0, t_unpack = 0;  // last call, microseconds
    ~HostBatchCtx() {
        release();
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void release() {  // (idle: every call completed before returning)
        map_cache().release(device, stage, cap);
        map_cache().release(device, h_tiles, tile_cap * sizeof(Tile));
        stage = stage_dev = nullptr;
        h_tiles = d_tiles = nullptr;
        cap = tile_cap = 0;
    }
    int reserve(int dev, size_t bytes, size_t tiles) {
        if (device != dev) {  // (events and mapped addresses are per device)
            release();
            for (hipEvent_t &e : ev)
                if (e) {
                    (void)hipEventDestroy(e);
                    e = nullptr;
                }
            device = dev;
        }
        if (cap < bytes) {
            map_cache().release(device, stage, cap);
            stage = stage_dev = nullptr;
            cap = 0;
            const size_t want = std::max(bytes, kHbStage);
            stage = static_cast<uint8_t *>(map_cache().acquire(dev, want));
            if (!stage) return fail(CEC_ENOMEM, "cec_region_multiply_batch: %zu bytes of mapped staging", want);
            cap = want;
            HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&stage_dev), stage, 0));
        }
        if (tile_cap < tiles) {
            // the tile list lives in mapped pinned memory too: the kernel's scalar loads read
            // it over PCIe, so a round needs no copy of it (one DMA set-up less per call)
            map_cache().release(device, h_tiles, tile_cap * sizeof(Tile));
            h_tiles = d_tiles = nullptr;
            tile_cap = 0;
            const size_t want = std::max(tiles, kHbStage / kTile * 2 + 1024);
            h_tiles = static_cast<Tile *>(map_cache().acquire(dev, want * sizeof(Tile)));
            if (!h_tiles) return fail(CEC_ENOMEM, "cec_region_multiply_batch: tile list of %zu", want);
            tile_cap = want;
            HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&d_tiles), h_tiles, 0));
        }
        if (!pool) pool.reset(new PackPool(pack_threads() - 1));
        return CEC_OK;
    }
};
thread_local HostBatchCtx t_hb;

// The streams of one round, the same slots in every round (the patterns are built once per
// batch): D, addressed by tile.off; S; B.
struct HbStreams {
    Streams st;
    int d, s, b;
    HbStreams(uint8_t *D, uint8_t *S, uint8_t *B) : d(st.add(D)), s(st.add(S)), b(st.add(B)) {}
};

inline bool ranges_meet(uintptr_t a, size_t na, uintptr_t b, size_t nb) { return a < b + nb && b < a + na; }

}  // namespace

CEC_API int cec_region_multiply_batch_stats(cec_batch_stats *out) {
    if (!out) return fail(CEC_EINVAL, "cec_region_multiply_batch_stats: out is NULL");
    out->launches = t_hb.last_launches;
    out->in_place_launches = t_hb.last_in_place;
    out->rounds = t_hb.last_rounds;
    out->plan_us = static_cast<float>(t_hb.t_plan);
    out->pack_us = static_cast<float>(t_hb.t_pack);
    out->gpu_us = static_cast<float>(t_hb.t_gpu);
    out->unpack_us = static_cast<float>(t_hb.t_unpack);
    return CEC_OK;
}

CEC_API int cec_region_multiply_batch(const cec_region_job *jobs, int n, void *stream) {
    using clk = std::chrono::steady_clock;
    auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    const clk::time_point t_start = clk::now();
    t_hb.last_launches = t_hb.last_rounds = t_hb.last_in_place = 0;
    t_hb.t_plan = t_hb.t_pack = t_hb.t_gpu = t_hb.t_unpack = 0;
    if (n < 0 || (n > 0 && !jobs)) return fail(CEC_EINVAL, "cec_region_multiply_batch: bad args");
    for (int i = 0; i < n; ++i) {
        const cec_region_job &j = jobs[i];
        if (j.multby < 0 || j.multby > 255 || (j.add != 0 && j.add != 1) || (j.base && !j.add) ||
            (j.len && (!j.src || !j.dst)))
            return fail(CEC_EINVAL, "cec_region_multiply_batch: job %d: multby %d add %d base %p src %p dst %p",
                        i, j.multby, j.add, j.base, j.src, j.dst);
    }
    // pieces
    std::vector<HbPiece> pc;
    pc.reserve(n);
    for (int i = 0; i < n; ++i) {
        const cec_region_job &j = jobs[i];
        if (!j.len) continue;
        const uint8_t *base = static_cast<const uint8_t *>(j.base);
        if (base == j.dst) base = nullptr;  // dst ^= c*src in place
        const uint8_t kind = !j.add ? kHbWrite : base ? kHbBase : kHbXor;
        if (kind == kHbXor && j.multby == 0) continue;  // adds nothing
        for (uint64_t o = 0; o < j.len; o += kHbPiece) {  // (64-bit: len may reach 2^32 - 1)
            HbPiece p{};
            p.src = static_cast<const uint8_t *>(j.src) + o;
            p.base = base ? base + o : nullptr;
            p.dst = static_cast<uint8_t *>(j.dst) + o;
            p.len = static_cast<uint32_t>(std::min<size_t>(kHbPiece, j.len - o));
            p.kind = kind;
            p.multby = static_cast<uint8_t>(j.multby);
            p.job = i;
            pc.push_back(p);
        }
    }
    if (pc.empty()) return CEC_OK;
    int dev;
    if (int r = current_device(&dev)) return r;
    // clusters of overlapping dst ranges, in address order (a radix sort: a comparison sort
    // of 65,536 scattered addresses costs milliseconds, as in the drainer)
    std::vector<int> ids(pc.size());
    {
        std::vector<std::pair<uint64_t, int>> key(pc.size());
        for (size_t i = 0; i < pc.size(); ++i) key[i] = {reinterpret_cast<uintptr_t>(pc[i].dst), static_cast<int>(i)};
        hb_radix_sort(key);
        for (size_t i = 0; i < pc.size(); ++i) ids[i] = key[i].second;
    }
    std::vector<HbCluster> cl;
    for (size_t x = 0; x < ids.size(); ++x) {
        const HbPiece &p = pc[ids[x]];
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p.dst), hi = lo + p.len;
        if (cl.empty() || lo >= cl.back().hi) {
            cl.push_back(HbCluster{lo, hi, static_cast<int>(x), 0, false, 1, 0});
        } else {
            cl.back().hi = std::max(cl.back().hi, hi);
        }
        ++cl.back().count;
        pc[ids[x]].cluster = static_cast<int>(cl.size()) - 1;
    }
    // sources and bases are read before anything is written: they must not meet a dst
    // (a base equal to its own dst was turned into an in-place XOR above).  One sweep of the
    // read ranges, sorted by start, over the disjoint sorted clusters: a read [a, a+l) meets
    // a dst iff the first cluster ending after a starts before a+l.
    {
        std::vector<std::pair<uint64_t, int>> rd;  // (start, piece * 2 + is_base)
        rd.reserve(2 * pc.size());
        for (size_t i = 0; i < pc.size(); ++i) {
            rd.emplace_back(reinterpret_cast<uintptr_t>(pc[i].src), static_cast<int>(2 * i));
            if (pc[i].base) rd.emplace_back(reinterpret_cast<uintptr_t>(pc[i].base), static_cast<int>(2 * i + 1));
        }
        hb_radix_sort(rd);
        size_t c = 0;
        for (const auto &x : rd) {
            const HbPiece &p = pc[x.second / 2];
            while (c < cl.size() && cl[c].hi <= x.first) ++c;
            if (c < cl.size() && ranges_meet(x.first, p.len, cl[c].lo, cl[c].hi - cl[c].lo))
                return fail(CEC_EOVERLAP, "cec_region_multiply_batch: job %d reads bytes a job writes", p.job);
        }
    }
    for (HbCluster &c : cl) c.waves = hb_cluster_waves(pc, ids.data() + c.first, c.count, &c.packed);
    // patterns: one per distinct (kind, multby) of the batch, in key order (the table set is
    // cached by content).  combos_ip: the same patterns for rounds that read their bases in
    // place: S by tile.off (it mirrors D), B by tile.src_off (the base's offset in its
    // registered region)
    const HbStreams slots(nullptr, nullptr, nullptr);  // (the slots alone)
    auto hb_combo = [&](int kind, int multby, bool in_place) {
        Combo cb;
        Combo::Out &o = cb.out(slots.d, kind == kHbXor ? kModeXor : kModeWrite);
        o.coef[cb.in(slots.s, !in_place)] = multby;
        if (kind == kHbBase) o.coef[cb.in(slots.b, true)] = 1;
        return cb;
    };
    std::vector<int> pat_of(3 * 256, -1);
    for (const HbPiece &p : pc) pat_of[p.kind * 256 + p.multby] = 0;
    std::vector<Combo> combos, combos_ip;
    for (int key = 0; key < 3 * 256; ++key) {
        if (pat_of[key] < 0) continue;
        pat_of[key] = static_cast<int>(combos.size());
        combos.push_back(hb_combo(key >> 8, key & 255, false));
        combos_ip.push_back(hb_combo(key >> 8, key & 255, true));
    }
    for (HbPiece &p : pc) p.pat = pat_of[p.kind * 256 + p.multby];
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (stream_capturing(s))  // a synchronous call: it waits for its own launches
        return fail(CEC_EINVAL, "cec_region_multiply_batch: the stream is being captured into a graph");
    HostBatchCtx &hb = t_hb;
    hb.t_plan = us(t_start, clk::now());
    auto a16 = [](uint64_t v, uintptr_t phase) { return v + ((phase - v) & 15); };  // next v' = phase (mod 16)
    auto r4k = [](uint64_t v) { return (v + kTile - 1) / kTile * kTile; };
    // Rounds: consecutive clusters within a staging half.  A batch that needs more than
    // kHbPipeMin of staging is cut into at least kHbPipeRounds rounds, so that the host packs
    // round r+1 and unpacks round r-1 while the GPU runs round r (two halves of staging).
    struct Round {
        size_t next, end;
        uint64_t dseg, sseg, tiles;
        bool any_base;
        bool in_place = false;  // bases read in place from reg (layout: S mirrors D, B by src_off)
        HostRegion reg;
    };
    uint64_t total_need = 0;
    for (const HbCluster &c : cl) {
        total_need += (c.hi - c.lo) + 32;
        for (int x = 0; x < c.count; ++x) {
            const HbPiece &p = pc[ids[c.first + x]];
            total_need += (p.kind == kHbBase ? 2u : 1u) * (p.len + 16);
        }
    }
    const uint64_t half_cap = total_need <= kHbPipeMin
                                  ? kHbStage
                                  : std::min<uint64_t>(kHbStage, std::max<uint64_t>(kHbPipeMin / 2,
                                                                                     total_need / kHbPipeRounds));
    const uint64_t tile_cap = kHbStage / kTile * 2 + 1024;
    std::vector<Round> rounds;
    uint64_t max_half = 0, max_tiles = 0;
    for (size_t next = 0; next < cl.size();) {
        Round rd{next, next, 0, 0, 0, false};
        uint64_t dsz = 0, ssz = 0, tiles = 0;
        bool any_base = false;
        size_t end = next;
        for (; end < cl.size(); ++end) {
            const HbCluster &c = cl[end];
            uint64_t d = a16(dsz, c.lo) + (c.hi - c.lo), sz = ssz, t = tiles;
            bool base = any_base;
            for (int x = 0; x < c.count; ++x) {
                const HbPiece &p = pc[ids[c.first + x]];
                sz = a16(sz, reinterpret_cast<uintptr_t>(p.dst)) + p.len;
                t += tiles_of(reinterpret_cast<uintptr_t>(p.dst) - c.lo + (a16(dsz, c.lo)), p.len);
                base |= p.kind == kHbBase;
            }
            const uint64_t need = r4k(d) + r4k(sz) * (base ? 2 : 1);
            if (end > next && (need > half_cap || t > tile_cap)) break;  // (one cluster always fits: grows)
            dsz = d;
            ssz = sz;
            tiles = t;
            any_base = base;
        }
        rd.end = end;
        rd.dseg = r4k(dsz);
        rd.sseg = r4k(ssz);
        rd.tiles = tiles;
        rd.any_base = any_base;
        // in place: one piece per cluster (so S can mirror D's offsets) and every base inside
        // one registered region
        if (any_base) {
            bool ok = true, have = false;
            for (size_t ci = next; ci < end && ok; ++ci) {
                const HbCluster &c = cl[ci];
                if (c.count != 1) {
                    ok = false;
                    break;
                }
                const HbPiece &p = pc[ids[c.first]];
                if (p.kind != kHbBase) continue;
                const uintptr_t b = reinterpret_cast<uintptr_t>(p.base);
                if (have) ok = b >= rd.reg.lo && b + p.len <= rd.reg.hi;
                else ok = have = host_region_find(b, p.len, dev, &rd.reg);
            }
            rd.in_place = ok && have;
        }
        max_half = std::max<uint64_t>(max_half, rd.dseg + rd.sseg * (any_base ? 2 : 1));
        max_tiles = std::max<uint64_t>(max_tiles, tiles);
        rounds.push_back(rd);
        next = end;
    }
    const bool piped = rounds.size() > 1;
    // (half 1 starts at stage + half: a 4 KiB multiple keeps it 16-B aligned, which the a16
    // phases above assume -- total_need / kHbPipeRounds alone is not, and every odd round's
    // pieces would miss the kernel's 16-B path)
    const uint64_t half = r4k(piped ? std::max<uint64_t>(max_half, half_cap) : max_half);
    const uint64_t tile_half = std::max<uint64_t>(max_tiles, piped ? tile_cap : 0);
    if (int r = hb.reserve(dev, piped ? 2 * half : half, piped ? 2 * tile_half : tile_half)) return r;
    if (piped) {
        for (int h = 0; h < 2; ++h)
            if (!hb.ev[h]) HIP_TRY(hipEventCreateWithFlags(&hb.ev[h], hipEventDisableTiming | hipEventReleaseToSystem));
    }
    std::vector<HbCopy> in, out[2];
    // lay round r out in half h, pack it, launch it (and record its event when piped)
    auto issue = [&](const Round &rd, int h) -> int {
        uint8_t *stage = hb.stage + h * half, *stage_dev = hb.stage_dev + h * half;
        Tile *ht = hb.h_tiles + h * tile_half, *dt = hb.d_tiles + h * tile_half;
        if ((reinterpret_cast<uintptr_t>(stage) | reinterpret_cast<uintptr_t>(stage_dev)) & 15)
            return fail(CEC_EINVAL, "cec_region_multiply_batch: staging half %d is not 16-B aligned", h);
        in.clear();
        out[h].clear();
        int max_wave = 0;
        uint64_t dcur = 0, scur = 0;
        for (size_t ci = rd.next; ci < rd.end; ++ci) {
            HbCluster &c = cl[ci];
            dcur = a16(dcur, c.lo);
            c.doff = dcur;
            dcur += c.hi - c.lo;
            if (c.packed) in.push_back(HbCopy{stage + c.doff, reinterpret_cast<const uint8_t *>(c.lo), c.hi - c.lo});
            out[h].push_back(HbCopy{reinterpret_cast<uint8_t *>(c.lo), stage + c.doff, c.hi - c.lo});
            max_wave = std::max(max_wave, c.waves);
            for (int x = 0; x < c.count; ++x) {
                HbPiece &p = pc[ids[c.first + x]];
                if (rd.in_place) {  // S at D's offset; B (if any) read in place at src_off
                    in.push_back(HbCopy{stage + rd.dseg + c.doff, p.src, p.len});
                    p.soff = p.base ? reinterpret_cast<uintptr_t>(p.base) - rd.reg.lo : 0;
                    continue;
                }
                scur = a16(scur, reinterpret_cast<uintptr_t>(p.dst));
                p.soff = scur;
                scur += p.len;
                in.push_back(HbCopy{stage + rd.dseg + p.soff, p.src, p.len});
                if (p.kind == kHbBase) in.push_back(HbCopy{stage + rd.dseg + rd.sseg + p.soff, p.base, p.len});
            }
        }
        std::vector<size_t> span(max_wave + 1, 0);  // tiles of wave w: [span[w], span[w+1])
        {
            std::vector<std::vector<int>> by_wave(max_wave);
            for (size_t ci = rd.next; ci < rd.end; ++ci)
                for (int x = 0; x < cl[ci].count; ++x) by_wave[pc[ids[cl[ci].first + x]].wave].push_back(ids[cl[ci].first + x]);
            size_t nt = 0;
            for (int w = 0; w < max_wave; ++w) {
                span[w] = nt;
                for (int id : by_wave[w]) {
                    const HbPiece &p = pc[id];
                    const HbCluster &c = cl[p.cluster];
                    nt += append_tiles(ht + nt, c.doff + (reinterpret_cast<uintptr_t>(p.dst) - c.lo), p.soff, p.len,
                                       static_cast<uint32_t>(p.pat));
                }
            }
            span[max_wave] = nt;
        }
        const clk::time_point t0 = clk::now();
        hb_copy(hb.pool.get(), in);
        hb.t_pack += us(t0, clk::now());
        const HbStreams hs(stage_dev, stage_dev + rd.dseg,  // D; S (by tile.src_off; in place: by tile.off)
                           rd.in_place ? rd.reg.alias       // B in place
                                       : rd.any_base ? stage_dev + rd.dseg + rd.sseg : stage_dev + rd.dseg);  // B staged
        for (int w = 0; w < max_wave; ++w) {
            if (span[w + 1] == span[w]) continue;
            const TileSource wave = TileSource::window(dt + span[w], ht + span[w], span[w + 1] - span[w]);
            if (int r = run_combos(dev, hs.st, rd.in_place ? combos_ip : combos, wave, s)) return r;
            ++hb.last_launches;
            hb.last_in_place += rd.in_place;
        }
        // (an event's completion carries the system-scope release of the kernels' writes
        // into the mapped staging: the host reads it after hipEventSynchronize)
        if (piped) HIP_TRY(hipEventRecord(hb.ev[h], s));
        ++hb.last_rounds;
        return CEC_OK;
    };
    auto drain = [&](int h) -> int {  // wait for half h's round, then copy its clusters out
        const clk::time_point t0 = clk::now();
        if (piped) {
            HIP_TRY(hipEventSynchronize(hb.ev[h]));
        } else if (int r = stream_wait(s, true)) {  // one round: the low-latency completion
            return r;
        }
        const clk::time_point t1 = clk::now();
        hb_copy(hb.pool.get(), out[h]);
        hb.t_gpu += us(t0, t1);
        hb.t_unpack += us(t1, clk::now());
        return CEC_OK;
    };
    // on a failure, nothing of this call may stay in flight: the staging is the thread's,
    // and its next call packs into it
    auto bail = [&](int rc) {
        (void)hipStreamSynchronize(s);
        (void)hipGetLastError();
        return rc;
    };
    for (size_t r = 0; r < rounds.size(); ++r) {
        const int h = static_cast<int>(r & 1);
        if (int rc = issue(rounds[r], h)) return bail(rc);
        if (r > 0)
            if (int rc = drain(h ^ 1)) return bail(rc);
    }
    if (int rc = drain(static_cast<int>((rounds.size() - 1) & 1))) return bail(rc);
    return CEC_OK;
}
