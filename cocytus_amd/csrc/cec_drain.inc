// cec_drain.inc -- the parity's deferred-commit drain (SURVEY §8f rank 1).
// Included by cec_runtime.hip (shares its launch internals); not a separate TU.
// From cec_hostplan.hpp: PackPool / split_copy (the pack) and overlap_waves (the address
// sort and the colouring).  From cec_cache.inc: Buf (every buffer), HalfPipe (the two
// staging halves), InFlight (a failed apply leaves nothing queued), classify.  From
// cec_runtime.hip: WaveTiles (a round's tile list and its launch windows).
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
//   * the fold is cec_apply_diffs' kernel (pattern j: parity ^= MATRIX(self, j) * diff);
//   * with live digests attached (cec_drainer_set_digests) each round ends with one
//     digest_update_kernel launch (cec_digest.inc) over the round's whole tile list, behind
//     its fold launches and reading the same staging: its atomics need no overlap waves;
//   * diffs received straight into the pinned staging area are folded from where they lie, and
//     a batch that mixes such diffs with others never packs over them (drainer_apply_mixed).
#include <memory>

constexpr size_t kRoundBytes = size_t(16) << 20;  // pipelining granularity

struct cec_drainer {
    int device = -1;
    int lid_self = 0;
    std::vector<int> matrix;
    Code code;  // over `matrix`
    size_t half = 0;       // staging bytes per half (>= the largest update)
    size_t tile_half = 0;  // tiles per half
    Buf h_stage, d_stage;  // pinned / device, 2 x half
    Buf h_tiles, d_tiles;  // pinned / device, 2 x tile_half tiles
    HalfPipe pipe;         // pinned half h is reusable once its event has fired
    std::unique_ptr<PackPool> pool;
    int last_launches = 0;
    Tracker uses;  // the streams of its applies (destroy waits for those only)
    // small windows (<= kDrainSmallBytes packed, <= kDrainSmallTiles tiles): packed by the
    // caller's thread into mapped pinned staging that the kernel reads in place, tile list
    // likewise, the low-latency completion -- no pack threads, no uploads (on first use)
    Buf sm, smt;
    // the parity's live digests (cec_drainer_set_digests; NULL: none), kept current by every apply
    uint8_t *digests = nullptr;
    uint64_t digest_limit = 0;  // n_units * 4096: no update may end beyond it
};

// cec_digest.inc
static int digest_limit(const char *op, uint64_t n_units, uint64_t *limit);
static int digest_update_launch(int dev, const Code &code, int lid_self, const uint8_t *diffs, uint8_t *digests,
                                const TileSource &src, hipStream_t stream);

constexpr size_t kDrainSmallBytes = size_t(1) << 20;
constexpr size_t kDrainSmallTiles = 8192;


CEC_API int cec_drainer_destroy(cec_drainer *d) {
    if (!d) return CEC_OK;
    (void)d->uses.wait(d->device);  // its own applies, not the device
    delete d;                       // (its buffers go back to the caches)
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
    const size_t tile_bytes = 2 * d->tile_half * sizeof(Tile);
    if (!d->h_stage.acquire(pin_cache(), dev, 2 * d->half) || !d->d_stage.acquire(dev_cache(), dev, 2 * d->half) ||
        !d->h_tiles.acquire(pin_cache(), dev, tile_bytes) || !d->d_tiles.acquire(dev_cache(), dev, tile_bytes) ||
        d->pipe.create(hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        cec_drainer_destroy(d);
        return fail(CEC_ENOMEM, "cec_drainer_create: staging allocation of 2 x %zu bytes", d->half);
    }
    d->pool.reset(new PackPool(pack_threads() - 1));
    *out = d;
    return CEC_OK;
}

CEC_API int cec_drainer_last_launches(const cec_drainer *d) { return d ? d->last_launches : 0; }

CEC_API int cec_drainer_set_digests(cec_drainer *d, uint8_t *digests, uint64_t n_units) {
    if (!d) return fail(CEC_EINVAL, "cec_drainer_set_digests: drainer is NULL");
    uint64_t limit = 0;
    if (digests) {
        if (reinterpret_cast<uintptr_t>(digests) & 15)
            return fail(CEC_EINVAL, "cec_drainer_set_digests: digests is not 16-byte aligned");
        if (int r = digest_limit("cec_drainer_set_digests", n_units, &limit)) return r;
    }
    d->digests = digests;
    d->digest_limit = limit;
    return CEC_OK;
}

CEC_API uint8_t *cec_drainer_staging(cec_drainer *d, size_t *capacity) {
    if (!d) return nullptr;
    if (capacity) *capacity = 2 * d->half;
    return d->h_stage.get();
}

// The per-update checks cec_drainer_apply makes before it touches anything (host only).
// *staged (where asked for, in the same pass): some non-empty update's buffer shares a byte
// with the staging area.
static int drainer_check(const cec_drainer *d, const cec_host_update *u, int n, const char *op,
                         bool *staged = nullptr) {
    if (!d || n < 0 || (n > 0 && !u)) return fail(CEC_EINVAL, "%s: bad args", op);
    if (staged) *staged = false;
    for (int i = 0; i < n; ++i) {
        if (staged && !*staged) *staged = meets_area(u[i].buf, u[i].len, d->h_stage.get(), 2 * d->half);
        if (u[i].src_lid >= static_cast<uint32_t>(d->code.k) || (u[i].len && !u[i].buf))
            return fail(CEC_EINVAL, "%s: update %d: src_lid %u / buf", op, i, u[i].src_lid);
        if (u[i].len > d->half)
            return fail(CEC_EINVAL, "%s: update %d (%u B) exceeds staging", op, i, u[i].len);
        if (d->digests && u[i].len && (u[i].addr > d->digest_limit || u[i].len > d->digest_limit - u[i].addr))
            return fail(CEC_EINVAL, "%s: update %d ends at %llu, beyond the attached digests' n_units * 4096 = %llu",
                        op, i, static_cast<unsigned long long>(u[i].addr + u[i].len),
                        static_cast<unsigned long long>(d->digest_limit));
    }
    return CEC_OK;
}

CEC_API int cec_drainer_validate(const cec_drainer *d, const cec_host_update *u, int n) {
    return drainer_check(d, u, n, "cec_drainer_validate");
}

// The fold launches of one round, one per overlap wave of `wt` (its tiles at dt on the
// device), then the round's digest update where digests are attached.  `stage`: the device
// address the tiles' src_off count from.
static int drainer_fold(cec_drainer *d, int dev, const uint8_t *stage, uint8_t *parity, const Tile *dt,
                        const WaveTiles &wt, hipStream_t s) {
    const Fold f = fold(d->code, d->lid_self, stage, parity);  // pattern j = source shard j
    for (int w = 0; w < wt.waves(); ++w) {
        const TileSource wave = wt.window(w, dt);
        if (!wave.n_tiles) continue;
        if (int r = run_combos(dev, f.st, f.combos, wave, s)) return r;
        ++d->last_launches;
    }
    if (d->digests && wt.n) {
        if (int r = digest_update_launch(dev, d->code, d->lid_self, stage, d->digests, wt.all(dt), s)) return r;
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
    Tile *ht = d->h_tiles.get<Tile>(), *dt = d->d_tiles.get<Tile>();
    size_t next = 0;
    while (next < order.size()) {
        WaveTiles wt(ht);
        while (next < order.size()) {
            const cec_host_update &x = u[order[next]];
            if (wt.n && wt.n + tiles_of(x.addr, x.len) > tcap) break;
            wt.enter(wave[order[next]]);
            wt.add(x.addr, static_cast<const uint8_t *>(x.buf) - d->h_stage.get(), x.len, x.src_lid);
            ++next;
        }
        HIP_TRY(hipMemcpyAsync(dt, ht, wt.n * sizeof(Tile), hipMemcpyHostToDevice, s));
        if (int r = drainer_fold(d, dev, d->d_stage.get(), parity, dt, wt, s)) return r;
        HIP_TRY(hipStreamSynchronize(s));  // the pinned tile list is reused by the next round
    }
    return CEC_OK;
}

// A small window, order[first, last) (the caller checked the bounds): one pass of the caller's
// thread packs the updates into the mapped staging and writes the tile list beside it; the
// kernel reads both in place; the completion is the signal-kernel spin (stream_wait), fenced
// when the arena is host memory (a registered ecmem).  Against the pack-thread path it saves
// the threads' wake-up, two uploads and a hipStreamSynchronize: ~15 us instead of ~45-60 per
// window.
static int drainer_apply_small(cec_drainer *d, const cec_host_update *u, const std::vector<int> &order,
                               size_t first, size_t last, const std::vector<int> &wave, uint8_t *parity, int dev,
                               hipStream_t s) {
    if (!d->smt && (!d->sm.acquire_mapped(dev, kDrainSmallBytes) ||
                    !d->smt.acquire_mapped(dev, kDrainSmallTiles * sizeof(Tile)))) {
        d->sm.release();
        return fail(CEC_ENOMEM, "cec_drainer_apply: small-window staging");
    }
    size_t so = 0;
    WaveTiles wt(d->smt.get<Tile>());
    for (size_t p = first; p < last; ++p) {
        const int i = order[p];
        const cec_host_update &x = u[i];
        wt.enter(wave[i]);
        if (x.len) memcpy(d->sm.get() + so, x.buf, x.len);
        wt.add(x.addr, so, x.len, x.src_lid);
        so += (x.len + 15) & ~static_cast<size_t>(15);
    }
    if (int r = drainer_fold(d, dev, d->sm.alias(), parity, d->smt.alias<Tile>(), wt, s)) return r;
    // the arena in host memory (registered), or unknown: fence the results
    return stream_wait(s, !classify(parity).device_memory());  // applied: the caller may ack / reuse its buffers
}

// The apply order of a batch: its overlap waves (wave[i]: update i's), then the list order.
static void wave_order(const cec_host_update *u, int n, std::vector<int> &wave, std::vector<int> &order) {
    const int n_waves = overlap_waves(u, n, wave);
    order.resize(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    if (n_waves > 1)
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return wave[a] < wave[b]; });
}

// A batch above the small window of which some diffs lie in the staging area and some do not.
// The pack path cannot take it: it packs into that very area, over diffs it has yet to read.
// Applied as two parts on the stream, each with its own waves (XOR accumulation commutes and
// the parts run in stream order, so the bytes are the sequential loop's): the diffs in the
// area in place, then the others through the small path's own mapped staging, one window of
// it after another.  Nothing is written to the staging area.  A mixed batch is the rare one
// (a diff too large for the receive buffers, malloc'd by the server): the windows complete one
// by one, without the pack path's overlap of copy and fold.
static int drainer_apply_mixed(cec_drainer *d, const cec_host_update *u, int n, uint8_t *parity, int dev,
                               hipStream_t s) {
    std::vector<cec_host_update> in, rest;
    uint64_t lo, hi;
    split_by_area(u, n, d->h_stage.get(), 2 * d->half, static_cast<uint32_t>(kDrainSmallBytes), in, rest, &lo, &hi);
    std::vector<int> wave, order;
    HIP_TRY(d->pipe.wait_all());
    if (hi > lo)  // (none wholly inside: a buffer that only partly lies in the area)
        HIP_TRY(hipMemcpyAsync(d->d_stage.get() + lo, d->h_stage.get() + lo, hi - lo, hipMemcpyHostToDevice, s));
    wave_order(in.data(), static_cast<int>(in.size()), wave, order);
    if (int r = drainer_apply_in_place(d, in.data(), order, wave, parity, dev, s)) return r;  // (synchronised)
    wave_order(rest.data(), static_cast<int>(rest.size()), wave, order);
    for (size_t next = 0; next < order.size();) {
        const size_t first = next;
        size_t bytes = 0, tiles = 0;
        for (; next < order.size(); ++next) {  // (a piece always fits: <= kDrainSmallBytes, so <= 257 tiles)
            const cec_host_update &x = rest[order[next]];
            bytes += (x.len + 15) & ~static_cast<size_t>(15);
            tiles += tiles_of(x.addr, x.len);
            if (next > first && (bytes > kDrainSmallBytes || tiles > kDrainSmallTiles)) break;
        }
        if (int r = drainer_apply_small(d, rest.data(), order, first, next, wave, parity, dev, s)) return r;
    }
    return CEC_OK;
}

CEC_API int cec_drainer_apply(cec_drainer *d, const cec_host_update *u, int n, uint8_t *parity,
                              void *stream) {
    if (!parity) return fail(CEC_EINVAL, "cec_drainer_apply: parity is NULL");
    bool staged;
    if (int r = drainer_check(d, u, n, "cec_drainer_apply", &staged)) return r;
    d->last_launches = 0;
    if (n == 0) return CEC_OK;
    int dev;
    if (int r = current_device(&dev)) return r;
    if (dev != d->device) return fail(CEC_EINVAL, "drainer of device %d used on %d", d->device, dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    UseNote note_{d->uses, s};
    uint8_t *const h_stage = d->h_stage.get(), *const d_stage = d->d_stage.get();
    // Updates already in the pinned staging area (received there): start their H2D now,
    // so it overlaps the wave colouring and tile building below.
    bool in_place = true;
    uint64_t lo = UINT64_MAX, hi = 0;
    for (int i = 0; i < n && in_place; ++i) {
        if (!u[i].len) continue;
        const uint8_t *b = static_cast<const uint8_t *>(u[i].buf);
        in_place = inside_area(b, u[i].len, h_stage, 2 * d->half);
        lo = std::min<uint64_t>(lo, b - h_stage);
        hi = std::max<uint64_t>(hi, b - h_stage + u[i].len);
    }
    // From here on the call enqueues work that reads the staging and the tile lists: on any
    // failed exit nothing of it stays in flight, and no half stays marked pending.
    InFlight guard(s, &d->pipe);
    if (in_place) {
        HIP_TRY(d->pipe.wait_all());
        if (hi > lo) HIP_TRY(hipMemcpyAsync(d_stage + lo, h_stage + lo, hi - lo, hipMemcpyHostToDevice, s));
    }
    std::vector<int> wave, order;
    wave_order(u, n, wave, order);

    if (in_place) {
        if (int r = drainer_apply_in_place(d, u, order, wave, parity, dev, s)) return r;
        guard.dismiss();
        return CEC_OK;
    }
    {
        size_t bytes = 0, tiles = 0;
        for (int i = 0; i < n && bytes <= kDrainSmallBytes && tiles <= kDrainSmallTiles; ++i) {
            bytes += (u[i].len + 15) & ~static_cast<size_t>(15);
            tiles += tiles_of(u[i].addr, u[i].len);
        }
        if (bytes <= kDrainSmallBytes && tiles <= kDrainSmallTiles) {
            if (int r = drainer_apply_small(d, u, order, 0, order.size(), wave, parity, dev, s)) return r;
            guard.dismiss();
            return CEC_OK;
        }
    }
    // The pack path writes the staging area: no diff it has yet to read may lie there.
    if (staged) {
        if (int r = drainer_apply_mixed(d, u, n, parity, dev, s)) return r;
        guard.dismiss();
        return CEC_OK;
    }

    std::vector<CopyItem> items;
    const size_t round_cap = std::min(d->half, std::max(kRoundBytes, static_cast<size_t>(kTile)));
    size_t next = 0;
    int h = 0;
    while (next < order.size()) {
        HIP_TRY(d->pipe.wait(h));
        uint8_t *hs = h_stage + h * d->half;
        Tile *ht = d->h_tiles.get<Tile>() + h * d->tile_half, *dt = d->d_tiles.get<Tile>() + h * d->tile_half;
        size_t so = 0;
        WaveTiles wt(ht);
        items.clear();
        while (next < order.size()) {
            const cec_host_update &x = u[order[next]];
            const size_t need = (x.len + 15) & ~static_cast<size_t>(15);
            // a round holds <= round_cap bytes, except that one update always fits
            if (!items.empty() && (so + need > round_cap || wt.n + tiles_of(x.addr, x.len) > d->tile_half)) break;
            wt.enter(wave[order[next]]);
            items.push_back(CopyItem{hs + so, static_cast<const uint8_t *>(x.buf), x.len});
            wt.add(x.addr, h * d->half + so, x.len, x.src_lid);  // (src_off relative to the whole staging area)
            so += need;
            ++next;
        }
        split_copy(d->pool.get(), items, 0);
        HIP_TRY(hipMemcpyAsync(d_stage + h * d->half, hs, so, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(dt, ht, wt.n * sizeof(Tile), hipMemcpyHostToDevice, s));
        HIP_TRY(d->pipe.record(h, s));  // pinned half h reusable once this fires
        if (int r = drainer_fold(d, dev, d_stage, parity, dt, wt, s)) return r;
        h ^= 1;
    }
    HIP_TRY(hipStreamSynchronize(s));  // applied: the caller may ack / reuse its buffers
    d->pipe.forget();
    guard.dismiss();
    return CEC_OK;
}
