// cec_drain.inc -- the parity's deferred-commit drain (SURVEY §8f rank 1).
// Included by cec_runtime.hip (shares its launch internals); not a separate TU.
//
// The parity side of a SET (process_rep_command, memcached.c:7739-7767) applies one
// shipped diff per call inside the drain loops (memcached.c:4231, 4322, 4350, 8068).
// cec_drainer_apply applies a whole batch of pending diffs that sit in host memory:
//   * updates are ordered into overlap-free waves (greedy interval colouring), so no
//     two lanes ever read-modify-write one parity byte in the same launch; XOR
//     accumulation commutes, so the result equals the sequential loop's;
//   * the ordered list is cut into rounds of <= kRoundBytes; a pool of host threads
//     packs round r into one half of a double-buffered pinned staging area while the
//     H2D copy and the fold kernel of round r-1 (other half) run on the stream;
//   * the fold is cec_apply_diffs' kernel (pattern j: parity ^= MATRIX(self, j) * diff).
#include <condition_variable>
#include <functional>
#include <memory>
#include <thread>

namespace {

// Persistent host threads for packing; run(fn) calls fn(t) for every t in
// [0, size()) (t = 0 on the caller) and returns when all have finished.
class PackPool {
  public:
    explicit PackPool(int workers) {
        for (int i = 0; i < workers; ++i) threads_.emplace_back([this, i] { loop(i + 1); });
    }
    ~PackPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : threads_) t.join();
    }
    int size() const { return static_cast<int>(threads_.size()) + 1; }
    void run(const std::function<void(int)> &fn) {
        if (threads_.empty()) {
            fn(0);
            return;
        }
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &fn;
            pending_ = threads_.size();
            ++gen_;
        }
        cv_.notify_all();
        fn(0);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return pending_ == 0; });
        job_ = nullptr;
    }

  private:
    void loop(int t) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)> *job;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                job = job_;
            }
            (*job)(t);
            std::lock_guard<std::mutex> lk(mu_);
            if (--pending_ == 0) done_.notify_one();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int)> *job_ = nullptr;
    uint64_t gen_ = 0;
    size_t pending_ = 0;
    bool stop_ = false;
};

constexpr size_t kRoundBytes = size_t(16) << 20;  // pipelining granularity

int pack_threads() {
    if (const char *e = getenv("CEC_PACK_THREADS")) return std::max(1, atoi(e));
    const unsigned hw = std::thread::hardware_concurrency();
    return static_cast<int>(std::max(1u, std::min(8u, hw / 2)));
}

}  // namespace

struct cec_drainer {
    int device = -1;
    int lid_self = 0;
    std::vector<int> matrix;
    Code code;  // over `matrix`
    size_t half = 0;       // staging bytes per half (>= the largest update)
    size_t tile_half = 0;  // tiles per half
    uint8_t *h_stage = nullptr, *d_stage = nullptr;  // 2 x half
    Tile *h_tiles = nullptr, *d_tiles = nullptr;     // 2 x tile_half
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};
    std::unique_ptr<PackPool> pool;
    int last_launches = 0;
    Tracker uses;  // the streams of its applies (destroy waits for those only)
    // small windows (<= kDrainSmallBytes packed, <= kDrainSmallTiles tiles): packed by the
    // caller's thread into mapped pinned staging that the kernel reads in place, tile list
    // likewise, the low-latency completion -- no pack threads, no uploads (on first use)
    uint8_t *sm_h = nullptr, *sm_d = nullptr;
    Tile *smt_h = nullptr, *smt_d = nullptr;
};

constexpr size_t kDrainSmallBytes = size_t(1) << 20;
constexpr size_t kDrainSmallTiles = 8192;


CEC_API int cec_drainer_destroy(cec_drainer *d) {
    if (!d) return CEC_OK;
    (void)d->uses.wait(d->device);  // its own applies, not the device
    pin_cache().release(d->device, d->h_stage, 2 * d->half);
    dev_cache().release(d->device, d->d_stage, 2 * d->half);
    pin_cache().release(d->device, d->h_tiles, 2 * d->tile_half * sizeof(Tile));
    dev_cache().release(d->device, d->d_tiles, 2 * d->tile_half * sizeof(Tile));
    map_cache().release(d->device, d->sm_h, kDrainSmallBytes);
    map_cache().release(d->device, d->smt_h, kDrainSmallTiles * sizeof(Tile));
    for (hipEvent_t e : d->ev)
        if (e) (void)hipEventDestroy(e);
    delete d;
    return CEC_OK;
}

CEC_API int cec_drainer_release_stream(cec_drainer *d, void *stream) {
    if (!d) return fail(CEC_EINVAL, "cec_drainer_release_stream: drainer is NULL");
    if (hipError_t e = d->uses.release(d->device, static_cast<hipStream_t>(stream)); e != hipSuccess)
        return fail(CEC_EHIP, "cec_drainer_release_stream: %s", hipGetErrorString(e));
    return CEC_OK;
}

CEC_API int cec_drainer_create(cec_drainer **out, int k, int m, const int *matrix, int lid_self,
                               size_t staging_bytes) {
    if (!out) return fail(CEC_EINVAL, "cec_drainer_create: out is NULL");
    *out = nullptr;
    if (int r = check_code(k, m, matrix)) return r;
    if (lid_self < k || lid_self >= k + m || staging_bytes < kTile)
        return fail(CEC_EINVAL, "cec_drainer_create: bad lid_self %d / staging %zu", lid_self,
                    staging_bytes);
    int dev;
    if (int r = current_device(&dev)) return r;
    cec_drainer *d = new (std::nothrow) cec_drainer;
    if (!d) return fail(CEC_ENOMEM, "cec_drainer_create: host allocation");
    d->device = dev;
    d->lid_self = lid_self;
    d->code = Code::owned(d->matrix, k, m, matrix);
    d->half = (staging_bytes + 15) & ~static_cast<size_t>(15);
    d->tile_half = d->half / 16 + 1024;  // worst case: 16-byte updates, one tile each
    d->h_stage = static_cast<uint8_t *>(pin_cache().acquire(dev, 2 * d->half));
    d->d_stage = static_cast<uint8_t *>(dev_cache().acquire(dev, 2 * d->half));
    d->h_tiles = static_cast<Tile *>(pin_cache().acquire(dev, 2 * d->tile_half * sizeof(Tile)));
    d->d_tiles = static_cast<Tile *>(dev_cache().acquire(dev, 2 * d->tile_half * sizeof(Tile)));
    if (!d->h_stage || !d->d_stage || !d->h_tiles || !d->d_tiles ||
        hipEventCreateWithFlags(&d->ev[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev[1], hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        cec_drainer_destroy(d);
        return fail(CEC_ENOMEM, "cec_drainer_create: staging allocation of 2 x %zu bytes", d->half);
    }
    d->pool.reset(new PackPool(pack_threads() - 1));
    *out = d;
    return CEC_OK;
}

CEC_API int cec_drainer_last_launches(const cec_drainer *d) { return d ? d->last_launches : 0; }

CEC_API uint8_t *cec_drainer_staging(cec_drainer *d, size_t *capacity) {
    if (!d) return nullptr;
    if (capacity) *capacity = 2 * d->half;
    return d->h_stage;
}

// The per-update checks cec_drainer_apply makes before it touches anything (host only).
static int drainer_check(const cec_drainer *d, const cec_host_update *u, int n, const char *op) {
    if (!d || n < 0 || (n > 0 && !u)) return fail(CEC_EINVAL, "%s: bad args", op);
    for (int i = 0; i < n; ++i) {
        if (u[i].src_lid >= static_cast<uint32_t>(d->code.k) || (u[i].len && !u[i].buf))
            return fail(CEC_EINVAL, "%s: update %d: src_lid %u / buf", op, i, u[i].src_lid);
        if (u[i].len > d->half)
            return fail(CEC_EINVAL, "%s: update %d (%u B) exceeds staging", op, i, u[i].len);
    }
    return CEC_OK;
}

CEC_API int cec_drainer_validate(const cec_drainer *d, const cec_host_update *u, int n) {
    return drainer_check(d, u, n, "cec_drainer_validate");
}

// A failure after the first launch: the earlier waves may still read the drainer's staging
// and tile lists, which the next apply overwrites from the host -- nothing of this call may
// stay in flight (as cec_region_multiply_batch's bail).
static int drain_bail(hipStream_t s, int rc) {
    (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
    return rc;
}

// The fold launches of one round, one per overlap wave: `spans` are the waves' tile ranges
// in the round's tile list (dt on the device, ht the same tiles on the host).  `stage`: the
// device address the tiles' src_off count from.
static int drainer_fold(cec_drainer *d, int dev, const uint8_t *stage, uint8_t *parity, const Tile *dt,
                        const Tile *ht, const std::vector<std::pair<size_t, size_t>> &spans, hipStream_t s) {
    const Fold f = fold(d->code, d->lid_self, stage, parity);  // pattern j = source shard j
    for (const auto &sp : spans) {
        if (sp.second == sp.first) continue;
        const TileSource wave = TileSource::window(dt + sp.first, ht + sp.first, sp.second - sp.first);
        if (int r = run_combos(dev, f.st, f.combos, wave, s)) return drain_bail(s, r);
        ++d->last_launches;
    }
    return CEC_OK;
}

// All updates already inside the pinned staging area: no pack copy.  The caller has
// enqueued the H2D of the used span; the fold launches wave by wave (tile lists in
// rounds of the tile buffer's capacity).
static int drainer_apply_in_place(cec_drainer *d, const cec_host_update *u,
                                  const std::vector<int> &order, const std::vector<int> &wave,
                                  uint8_t *parity, int dev, hipStream_t s) {
    const size_t tcap = 2 * d->tile_half;
    size_t next = 0;
    while (next < order.size()) {
        size_t nt = 0;
        std::vector<std::pair<size_t, size_t>> spans;
        int cur_wave = -1;
        while (next < order.size()) {
            const cec_host_update &x = u[order[next]];
            const size_t tiles = tiles_of(x.addr, x.len);
            if (nt && nt + tiles > tcap) break;
            if (wave[order[next]] != cur_wave) {
                cur_wave = wave[order[next]];
                spans.emplace_back(nt, nt);
            }
            const uint64_t so = static_cast<const uint8_t *>(x.buf) - d->h_stage;
            nt += append_tiles(d->h_tiles + nt, x.addr, so, x.len, x.src_lid);
            spans.back().second = nt;
            ++next;
        }
        HIP_TRY(hipMemcpyAsync(d->d_tiles, d->h_tiles, nt * sizeof(Tile), hipMemcpyHostToDevice, s));
        if (int r = drainer_fold(d, dev, d->d_stage, parity, d->d_tiles, d->h_tiles, spans, s)) return r;
        HIP_TRY(hipStreamSynchronize(s));  // the pinned tile list is reused by the next round
    }
    return CEC_OK;
}

// A small window (the caller checked the bounds): one pass of the caller's thread packs the
// updates into the mapped staging and writes the tile list beside it; the kernel reads both
// in place; the completion is the signal-kernel spin (stream_wait), fenced when the arena is
// host memory (a registered ecmem).  Against the pack-thread path it saves the threads'
// wake-up, two uploads and a hipStreamSynchronize: ~15 us instead of ~45-60 per window.
static int drainer_apply_small(cec_drainer *d, const cec_host_update *u, const std::vector<int> &order,
                               const std::vector<int> &wave, uint8_t *parity, int dev, hipStream_t s) {
    if (!d->sm_h) {
        d->sm_h = static_cast<uint8_t *>(map_cache().acquire(dev, kDrainSmallBytes));
        d->smt_h = static_cast<Tile *>(map_cache().acquire(dev, kDrainSmallTiles * sizeof(Tile)));
        if (!d->sm_h || !d->smt_h ||
            hipHostGetDevicePointer(reinterpret_cast<void **>(&d->sm_d), d->sm_h, 0) != hipSuccess ||
            hipHostGetDevicePointer(reinterpret_cast<void **>(&d->smt_d), d->smt_h, 0) != hipSuccess) {
            (void)hipGetLastError();
            map_cache().release(dev, d->sm_h, kDrainSmallBytes);
            map_cache().release(dev, d->smt_h, kDrainSmallTiles * sizeof(Tile));
            d->sm_h = d->sm_d = nullptr;
            d->smt_h = d->smt_d = nullptr;
            return fail(CEC_ENOMEM, "cec_drainer_apply: small-window staging");
        }
    }
    size_t so = 0, nt = 0;
    std::vector<std::pair<size_t, size_t>> spans;
    int cur_wave = -1;
    for (int i : order) {
        const cec_host_update &x = u[i];
        if (wave[i] != cur_wave) {
            cur_wave = wave[i];
            spans.emplace_back(nt, nt);
        }
        if (x.len) memcpy(d->sm_h + so, x.buf, x.len);
        nt += append_tiles(d->smt_h + nt, x.addr, so, x.len, x.src_lid);
        spans.back().second = nt;
        so += (x.len + 15) & ~static_cast<size_t>(15);
    }
    if (int r = drainer_fold(d, dev, d->sm_d, parity, d->smt_d, d->smt_h, spans, s)) return r;
    hipPointerAttribute_t at;  // the arena in host memory (registered): fence the results
    bool host = true;
    if (hipPointerGetAttributes(&at, parity) == hipSuccess)
        host = at.type != hipMemoryTypeDevice;
    else
        (void)hipGetLastError();
    return stream_wait(s, host);  // applied: the caller may ack / reuse its buffers
}

// Updates by arena address: LSD radix sort of (addr, index) pairs, 11-bit digits, digits
// on which every address agrees skipped (an 8 GiB arena: at most 3 passes).  For 65,536
// shuffled updates it took 1.1 ms where std::sort through the index took 5.7 on the build
// host (DESIGN.md §5): the colouring runs before the pack path can start.
static void sort_by_addr(const cec_host_update *u, int n, std::vector<std::pair<uint64_t, int>> &a) {
    a.resize(n);
    uint64_t orv = 0, andv = ~0ull;
    for (int i = 0; i < n; ++i) {
        a[i] = {u[i].addr, i};
        orv |= u[i].addr;
        andv &= u[i].addr;
    }
    const uint64_t varies = orv ^ andv;
    std::vector<std::pair<uint64_t, int>> b(n);
    for (int shift = 0; shift < 64; shift += 11) {
        if (((varies >> shift) & 0x7FF) == 0) continue;
        size_t cnt[2049] = {};
        for (const auto &x : a) ++cnt[((x.first >> shift) & 0x7FF) + 1];
        for (int d = 0; d < 2048; ++d) cnt[d + 1] += cnt[d];
        for (const auto &x : a) b[cnt[(x.first >> shift) & 0x7FF]++] = x;  // stable
        a.swap(b);
    }
}

// Greedy interval colouring of [addr, addr+len): wave[i] = lowest wave with no
// overlapping member.  Sorted sweep with a min-heap of (end, wave) of open ranges; when no
// two updates overlap (the usual batch: distinct values), one linear pass over the sorted
// order proves it and every update is in wave 0.  Returns the number of waves.
static int overlap_waves(const cec_host_update *u, int n, std::vector<int> &wave) {
    std::vector<std::pair<uint64_t, int>> byaddr;
    sort_by_addr(u, n, byaddr);
    wave.assign(n, 0);
    {
        uint64_t end = 0;
        bool overlap = false;
        for (const auto &x : byaddr) {
            const cec_host_update &v = u[x.second];
            if (!v.len) continue;
            if (v.addr < end) {
                overlap = true;
                break;
            }
            end = std::max<uint64_t>(end, v.addr + v.len);
        }
        if (!overlap) return 1;
    }
    std::vector<std::pair<uint64_t, int>> open;  // min-heap on end
    std::vector<int> free_waves;
    int nw = 0;
    auto cmp = [](const std::pair<uint64_t, int> &a, const std::pair<uint64_t, int> &b) {
        return a.first > b.first;
    };
    for (const auto &x : byaddr) {
        const int i = x.second;
        while (!open.empty() && open.front().first <= u[i].addr) {
            free_waves.push_back(open.front().second);
            std::pop_heap(open.begin(), open.end(), cmp);
            open.pop_back();
        }
        int w;
        if (!free_waves.empty()) {
            auto it = std::min_element(free_waves.begin(), free_waves.end());
            w = *it;
            free_waves.erase(it);
        } else {
            w = nw++;
        }
        wave[i] = w;
        if (u[i].len) {
            open.emplace_back(u[i].addr + u[i].len, w);
            std::push_heap(open.begin(), open.end(), cmp);
        } else {
            free_waves.push_back(w);
        }
    }
    return std::max(nw, 1);
}

CEC_API int cec_drainer_apply(cec_drainer *d, const cec_host_update *u, int n, uint8_t *parity,
                              void *stream) {
    if (!parity) return fail(CEC_EINVAL, "cec_drainer_apply: parity is NULL");
    if (int r = drainer_check(d, u, n, "cec_drainer_apply")) return r;
    d->last_launches = 0;
    if (n == 0) return CEC_OK;
    int dev;
    if (int r = current_device(&dev)) return r;
    if (dev != d->device) return fail(CEC_EINVAL, "drainer of device %d used on %d", d->device, dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    UseNote note_{d->uses, s};
    // Updates already in the pinned staging area (received there): start their H2D now,
    // so it overlaps the wave colouring and tile building below.
    bool in_place = true;
    uint64_t lo = UINT64_MAX, hi = 0;
    for (int i = 0; i < n && in_place; ++i) {
        if (!u[i].len) continue;
        const uint8_t *b = static_cast<const uint8_t *>(u[i].buf);
        in_place = b >= d->h_stage && b + u[i].len <= d->h_stage + 2 * d->half;
        lo = std::min<uint64_t>(lo, b - d->h_stage);
        hi = std::max<uint64_t>(hi, b - d->h_stage + u[i].len);
    }
    if (in_place) {
        for (int h = 0; h < 2; ++h)
            if (d->pending[h]) HIP_TRY(hipEventSynchronize(d->ev[h]));
        d->pending[0] = d->pending[1] = false;
        if (hi > lo)
            HIP_TRY(hipMemcpyAsync(d->d_stage + lo, d->h_stage + lo, hi - lo, hipMemcpyHostToDevice, s));
    }
    std::vector<int> wave;
    const int n_waves = overlap_waves(u, n, wave);
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    if (n_waves > 1)
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return wave[a] < wave[b]; });

    if (in_place) return drainer_apply_in_place(d, u, order, wave, parity, dev, s);
    {
        size_t bytes = 0, tiles = 0;
        for (int i = 0; i < n && bytes <= kDrainSmallBytes && tiles <= kDrainSmallTiles; ++i) {
            bytes += (u[i].len + 15) & ~static_cast<size_t>(15);
            tiles += tiles_of(u[i].addr, u[i].len);
        }
        if (bytes <= kDrainSmallBytes && tiles <= kDrainSmallTiles)
            return drainer_apply_small(d, u, order, wave, parity, dev, s);
    }

    struct Item {
        uint8_t *dst;
        const uint8_t *src;
        size_t len, prefix;
    };
    std::vector<Item> items;
    std::vector<std::pair<size_t, size_t>> spans;  // tile ranges of each wave in the round
    const size_t round_cap = std::min(d->half, std::max(kRoundBytes, static_cast<size_t>(kTile)));
    size_t next = 0;
    int h = 0;
    while (next < order.size()) {
        if (d->pending[h]) HIP_TRY(hipEventSynchronize(d->ev[h]));
        d->pending[h] = false;
        uint8_t *hs = d->h_stage + h * d->half;
        Tile *ht = d->h_tiles + h * d->tile_half;
        size_t so = 0, nt = 0;
        int cur_wave = -1;
        items.clear();
        spans.clear();
        while (next < order.size()) {
            const cec_host_update &x = u[order[next]];
            const size_t need = (x.len + 15) & ~static_cast<size_t>(15);
            const size_t tiles = tiles_of(x.addr, x.len);
            // a round holds <= round_cap bytes, except that one update always fits
            if (!items.empty() && (so + need > round_cap || nt + tiles > d->tile_half)) break;
            if (wave[order[next]] != cur_wave) {
                cur_wave = wave[order[next]];
                spans.emplace_back(nt, nt);
            }
            items.push_back(Item{hs + so, static_cast<const uint8_t *>(x.buf), x.len,
                                 items.empty() ? 0 : items.back().prefix + items.back().len});
            nt += append_tiles(ht + nt, x.addr, h * d->half + so, x.len, x.src_lid);
            spans.back().second = nt;
            so += need;
            ++next;
        }
        // pack: thread t copies bytes [t*B/T, (t+1)*B/T) of the concatenated updates
        const size_t total = items.back().prefix + items.back().len;
        const int T = d->pool->size();
        d->pool->run([&](int t) {
            const size_t lo = total * t / T, hi = total * (t + 1) / T;
            if (lo >= hi) return;
            size_t i = std::upper_bound(items.begin(), items.end(), lo,
                                        [](size_t v, const Item &it) { return v < it.prefix; }) -
                       items.begin() - 1;
            for (size_t pos = lo; pos < hi && i < items.size(); ++i) {
                const Item &it = items[i];
                const size_t a = pos - it.prefix, b = std::min(it.len, hi - it.prefix);
                if (b > a) memcpy(it.dst + a, it.src + a, b - a);
                pos = it.prefix + b;
            }
        });
        HIP_TRY(hipMemcpyAsync(d->d_stage + h * d->half, hs, so, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d->d_tiles + h * d->tile_half, ht, nt * sizeof(Tile),
                               hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(d->ev[h], s));  // pinned half h reusable once this fires
        d->pending[h] = true;
        // (tiles carry src_off relative to the whole staging area)
        if (int r = drainer_fold(d, dev, d->d_stage, parity, d->d_tiles + h * d->tile_half, ht, spans, s)) {
            d->pending[0] = d->pending[1] = false;
            return r;
        }
        h ^= 1;
    }
    HIP_TRY(hipStreamSynchronize(s));  // applied: the caller may ack / reuse its buffers
    d->pending[0] = d->pending[1] = false;
    return CEC_OK;
}
