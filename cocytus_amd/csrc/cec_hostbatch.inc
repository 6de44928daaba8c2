// cec_hostbatch.inc -- galois_w08_region_multiply, batched, over host memory.
// Included by cec_runtime.hip after cec_recovery.inc (shares stream_wait and the launch
// internals); not a separate TU.  The planning below the C-ABI -- HbPiece, HbCluster,
// MaxTree, hb_cluster_waves, radix_sort -- and PackPool / split_copy are in
// cec_hostplan.hpp; Buf, HalfPipe and InFlight in cec_cache.inc; WaveTiles in
// cec_runtime.hip.
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

struct HostBatchCtx {  // per thread and device
    int device = -1;
    Buf stage;  // mapped pinned
    // the tile list lives in mapped pinned memory too: the kernel's scalar loads read it
    // over PCIe, so a round needs no copy of it (one DMA set-up less per call)
    Buf tiles;
    HalfPipe pipe;  // round completion per staging half (pipelined batches)
    std::unique_ptr<PackPool> pool;
    int last_launches = 0, last_rounds = 0, last_in_place = 0;
    double t_plan = 0, t_pack = 0, t_gpu = 0, t_unpack = 0;  // last call, microseconds
    // (buffers are idle whenever they are released: every call completed before returning)
    int reserve(int dev, size_t bytes, size_t n_tiles) {
        if (device != dev) {  // (events and mapped addresses are per device)
            stage.release();
            tiles.release();
            pipe.destroy();
            device = dev;
        }
        if (stage.bytes() < bytes && !stage.acquire_mapped(dev, std::max(bytes, kHbStage)))
            return fail(CEC_ENOMEM, "cec_region_multiply_batch: %zu bytes of mapped staging", bytes);
        if (tiles.bytes() < n_tiles * sizeof(Tile) &&
            !tiles.acquire_mapped(dev, std::max(n_tiles, kHbStage / kTile * 2 + 1024) * sizeof(Tile)))
            return fail(CEC_ENOMEM, "cec_region_multiply_batch: tile list of %zu", n_tiles);
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
        radix_sort(key);
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
        radix_sort(rd);
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
    if (piped) HIP_TRY(hb.pipe.create(hipEventDisableTiming | hipEventReleaseToSystem));
    std::vector<CopyItem> in, out[2];
    // lay round r out in half h, pack it, launch it (and record its event when piped)
    auto issue = [&](const Round &rd, int h) -> int {
        uint8_t *stage = hb.stage.get() + h * half, *stage_dev = hb.stage.alias() + h * half;
        Tile *ht = hb.tiles.get<Tile>() + h * tile_half, *dt = hb.tiles.alias<Tile>() + h * tile_half;
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
            if (c.packed) in.push_back(CopyItem{stage + c.doff, reinterpret_cast<const uint8_t *>(c.lo), c.hi - c.lo});
            out[h].push_back(CopyItem{reinterpret_cast<uint8_t *>(c.lo), stage + c.doff, c.hi - c.lo});
            max_wave = std::max(max_wave, c.waves);
            for (int x = 0; x < c.count; ++x) {
                HbPiece &p = pc[ids[c.first + x]];
                if (rd.in_place) {  // S at D's offset; B (if any) read in place at src_off
                    in.push_back(CopyItem{stage + rd.dseg + c.doff, p.src, p.len});
                    p.soff = p.base ? reinterpret_cast<uintptr_t>(p.base) - rd.reg.lo : 0;
                    continue;
                }
                scur = a16(scur, reinterpret_cast<uintptr_t>(p.dst));
                p.soff = scur;
                scur += p.len;
                in.push_back(CopyItem{stage + rd.dseg + p.soff, p.src, p.len});
                if (p.kind == kHbBase) in.push_back(CopyItem{stage + rd.dseg + rd.sseg + p.soff, p.base, p.len});
            }
        }
        WaveTiles wt(ht);
        {
            std::vector<std::vector<int>> by_wave(max_wave);
            for (size_t ci = rd.next; ci < rd.end; ++ci)
                for (int x = 0; x < cl[ci].count; ++x) by_wave[pc[ids[cl[ci].first + x]].wave].push_back(ids[cl[ci].first + x]);
            for (int w = 0; w < max_wave; ++w) {
                wt.begin_wave();
                for (int id : by_wave[w]) {
                    const HbPiece &p = pc[id];
                    const HbCluster &c = cl[p.cluster];
                    wt.add(c.doff + (reinterpret_cast<uintptr_t>(p.dst) - c.lo), p.soff, p.len, static_cast<uint32_t>(p.pat));
                }
            }
        }
        const clk::time_point t0 = clk::now();
        split_copy(hb.pool.get(), in, kHbParallelCopy);
        hb.t_pack += us(t0, clk::now());
        const HbStreams hs(stage_dev, stage_dev + rd.dseg,  // D; S (by tile.src_off; in place: by tile.off)
                           rd.in_place ? rd.reg.alias       // B in place
                                       : rd.any_base ? stage_dev + rd.dseg + rd.sseg : stage_dev + rd.dseg);  // B staged
        for (int w = 0; w < max_wave; ++w) {
            const TileSource wave = wt.window(w, dt);
            if (!wave.n_tiles) continue;
            if (int r = run_combos(dev, hs.st, rd.in_place ? combos_ip : combos, wave, s)) return r;
            ++hb.last_launches;
            hb.last_in_place += rd.in_place;
        }
        // (an event's completion carries the system-scope release of the kernels' writes
        // into the mapped staging: the host reads it after hipEventSynchronize)
        if (piped) HIP_TRY(hb.pipe.record(h, s));
        ++hb.last_rounds;
        return CEC_OK;
    };
    auto drain = [&](int h) -> int {  // wait for half h's round, then copy its clusters out
        const clk::time_point t0 = clk::now();
        if (piped) {
            HIP_TRY(hb.pipe.wait(h));
        } else if (int r = stream_wait(s, true)) {  // one round: the low-latency completion
            return r;
        }
        const clk::time_point t1 = clk::now();
        split_copy(hb.pool.get(), out[h], kHbParallelCopy);
        hb.t_gpu += us(t0, t1);
        hb.t_unpack += us(t1, clk::now());
        return CEC_OK;
    };
    // on a failure, nothing of this call may stay in flight: the staging is the thread's,
    // and its next call packs into it
    InFlight guard(s, &hb.pipe);
    for (size_t r = 0; r < rounds.size(); ++r) {
        const int h = static_cast<int>(r & 1);
        if (int rc = issue(rounds[r], h)) return rc;
        if (r > 0)
            if (int rc = drain(h ^ 1)) return rc;
    }
    if (int rc = drain(static_cast<int>((rounds.size() - 1) & 1))) return rc;
    guard.dismiss();
    return CEC_OK;
}
