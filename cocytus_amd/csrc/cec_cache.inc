// cec_cache.inc -- completion tracking and the process-wide caches of libcocytus_ec.
// Included by cec_runtime.hip after the device state; not a separate TU.
//
// Nothing here may synchronise the whole device: a parity server runs many streams
// (drain, recovery, the drop-in) and a device-wide wait in one of them stalls all.
//   * Tracker: the streams an object (plan, session, drainer, pool) was used on; its
//     destroy synchronises those streams only, never the whole device.
//   * BufCache: idle device / pinned buffers kept for reuse.  hipFree and hipHostFree
//     wait for the device; releasing into the cache does not.  Sizes are bucketed at
//     <= 12.5 % waste and the cache is capped; cec_cache_trim() frees it.
//   * Buf, HalfPipe, InFlight, classify: what the ops hold the caches' buffers, their
//     two staging halves, their queued work and their callers' pointers with.
//   * PatternCache: coefficient tables per (device, content), LRU-bounded, uploaded
//     asynchronously from a pinned mirror on the first caller's stream; another stream
//     waits on the upload event (until it is known complete).  Tables used inside a
//     stream capture are uploaded before the capture continues and are never evicted
//     (the graph keeps their address).  Eviction (only past 4096 distinct sets by
//     default) synchronises the device once per batch of victims.
#include <list>
#include <memory>
#include <unordered_map>

namespace {

// ---------------------------------------------------------------- capture helpers
bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return st == hipStreamCaptureStatusActive;
}

// Allocation and host-side waits made while this thread captures a graph in global
// mode are "unsafe" calls; relaxed mode allows them (what torch's allocator does).
struct RelaxedCapture {
    bool on;
    hipStreamCaptureMode prev = hipStreamCaptureModeRelaxed;
    explicit RelaxedCapture(bool active = true) : on(active) {
        if (on) (void)hipThreadExchangeStreamCaptureMode(&prev);
    }
    ~RelaxedCapture() {
        if (on) (void)hipThreadExchangeStreamCaptureMode(&prev);
    }
};

// Hash of a coefficient-table key (1.7 KiB per pattern): 8 bytes a step, multiply-xorshift;
// std::hash<std::string> cost about a microsecond per drop-in call at this size.
struct KeyHash {
    size_t operator()(const std::string &k) const {
        uint64_t h = 0x9E3779B97F4A7C15ull ^ k.size();
        const char *p = k.data();
        size_t i = 0;
        for (; i + 8 <= k.size(); i += 8) {
            uint64_t w;
            memcpy(&w, p + i, 8);
            h = (h ^ w) * 0xBF58476D1CE4E5B9ull;
            h ^= h >> 29;
        }
        for (; i < k.size(); ++i) h = (h ^ static_cast<uint8_t>(p[i])) * 0x94D049BB133111EBull;
        return static_cast<size_t>(h ^ (h >> 32));
    }
};

// ---------------------------------------------------------------- completion tracking
// An object records, on the host, which streams it was used on -- nothing is added to
// a stream per launch (a completion event bound to every launch measured +3.7 us of
// idle GPU between back-to-back kernels, 1.9 % of the metric's step; an event recorded
// behind each launch cost more).  Before its memory is reused it synchronises exactly
// those streams (hipStreamSynchronize waits for the stream's own last command, so work
// of other streams -- even ones sharing its hardware queue -- is never waited for; a
// marker recorded at that moment would queue behind them).  Contract (cocytus_ec.h):
// an object is destroyed before the streams it was used on.
class Tracker {
  public:
    // No stream handle is queried here (a handle noted earlier may belong to a stream
    // another thread is capturing, which a query would invalidate): the list holds every
    // distinct stream used since the last wait, which the contract keeps alive.
    void note(hipStream_t s) {
        std::lock_guard<std::mutex> lk(mu_);
        for (hipStream_t x : streams_)
            if (x == s) return;
        streams_.push_back(s);
    }
    // Wait for everything queued so far on the streams this object was used on.
    hipError_t wait(int dev) {
        std::vector<hipStream_t> ss;
        {
            std::lock_guard<std::mutex> lk(mu_);
            ss.swap(streams_);
        }
        int cur = dev;
        (void)hipGetDevice(&cur);
        if (cur != dev) (void)hipSetDevice(dev);  // the null stream is per device
        hipError_t rc = hipSuccess;
        for (hipStream_t s : ss) {
            const hipError_t w = hipStreamSynchronize(s);
            if (w != hipSuccess && rc == hipSuccess) rc = w;
        }
        (void)hipGetLastError();
        if (cur != dev) (void)hipSetDevice(cur);
        return rc;
    }
    bool empty() {
        std::lock_guard<std::mutex> lk(mu_);
        return streams_.empty();
    }
    // The caller is about to destroy stream s (a closing connection's stream): wait for
    // what the object queued on it and drop it from the list, so the list stays bounded
    // by the streams alive and destroy never touches a dead handle.  Not listed: no-op.
    // A stream being captured cannot be waited for: refused, the list unchanged.
    hipError_t release(int dev, hipStream_t s) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (std::find(streams_.begin(), streams_.end(), s) == streams_.end()) return hipSuccess;
        }
        if (stream_capturing(s)) return hipErrorStreamCaptureUnsupported;
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto it = std::find(streams_.begin(), streams_.end(), s);
            if (it == streams_.end()) return hipSuccess;
            streams_.erase(it);
        }
        int cur = dev;
        (void)hipGetDevice(&cur);
        if (cur != dev) (void)hipSetDevice(dev);
        const hipError_t rc = hipStreamSynchronize(s);
        (void)hipGetLastError();
        if (cur != dev) (void)hipSetDevice(cur);
        return rc;
    }
    size_t size() {
        std::lock_guard<std::mutex> lk(mu_);
        return streams_.size();
    }

  private:
    std::mutex mu_;
    std::vector<hipStream_t> streams_;
};

// Notes a synchronous call's stream in an object's tracker when the call returns (on
// every path: an error can leave copies or launches queued).
struct UseNote {
    Tracker &t;
    hipStream_t s;
    ~UseNote() { t.note(s); }
};

// ---------------------------------------------------------------- buffer caches
// Bucket of a request: powers of two up to 64 KiB, then 8 steps per octave.
size_t cache_bucket(size_t bytes) {
    if (bytes <= 4096) return 4096;
    if (bytes <= 65536) {
        size_t b = 4096;
        while (b < bytes) b <<= 1;
        return b;
    }
    int e = 63 - __builtin_clzll(bytes);  // 2^e <= bytes < 2^(e+1)
    const size_t step = size_t(1) << (e - 3);
    return (bytes + step - 1) / step * step;
}

void register_exit_trim();  // (below)

enum BufKind { kBufDevice, kBufPinned, kBufMapped };  // hipMalloc / hipHostMalloc / mapped+coherent

class BufCache {
  public:
    BufCache(BufKind kind, size_t cap) : kind_(kind), cap_(cap) {}
    // A buffer of >= bytes on device dev (the current device); NULL if out of memory
    // even after the cache was trimmed.
    void *acquire(int dev, size_t bytes, size_t *got = nullptr) {
        const size_t b = cache_bucket(bytes);
        if (got) *got = b;
        {
            std::lock_guard<std::mutex> lk(mu_);
            auto it = bufs_.find({dev, b});
            if (it != bufs_.end()) {
                void *p = it->second;
                bufs_.erase(it);
                cached_ -= b;
                return p;
            }
        }
        void *p = alloc(b);
        if (!p && trim()) p = alloc(b);  // idle cached memory may be what is missing
        return p;
    }
    // p (from acquire(dev, bytes)) must be idle: the work that used it has completed.
    void release(int dev, void *p, size_t bytes) {
        if (!p) return;
        const size_t b = cache_bucket(bytes);
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (cached_ + b <= cap_) {
                bufs_.emplace(std::make_pair(dev, b), p);
                cached_ += b;
                return;
            }
        }
        dealloc(p);  // over the cap: a real free (may wait for the device)
    }
    size_t trim() {
        std::multimap<std::pair<int, size_t>, void *> all;
        {
            std::lock_guard<std::mutex> lk(mu_);
            all.swap(bufs_);
            cached_ = 0;
        }
        size_t n = 0;
        for (auto &x : all) {
            dealloc(x.second);
            n += x.first.second;
        }
        return n;
    }
    size_t cached() {
        std::lock_guard<std::mutex> lk(mu_);
        return cached_;
    }
    size_t cap() const { return cap_; }

  private:
    // Allocation and free go through one process-wide mutex: they are rare, and a buffer
    // freed by one thread and handed out again by the HIP allocator to another is then
    // ordered (memory reuse the host sanitizers can see; the HIP allocator is opaque).
    static std::mutex &alloc_mu() {
        static std::mutex *m = new std::mutex;
        return *m;
    }
    void *alloc(size_t b) {
        register_exit_trim();  // this process now holds buffers to give back at exit
        std::lock_guard<std::mutex> lk(alloc_mu());
        RelaxedCapture relax;
        void *p = nullptr;
        const hipError_t e =
            kind_ == kBufDevice ? hipMalloc(&p, b)
            : kind_ == kBufPinned ? hipHostMalloc(&p, b, hipHostMallocDefault)
                                  : hipHostMalloc(&p, b, hipHostMallocMapped | hipHostMallocCoherent);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        return p;
    }
    void dealloc(void *p) {
        std::lock_guard<std::mutex> lk(alloc_mu());
        RelaxedCapture relax;
        (void)(kind_ == kBufDevice ? hipFree(p) : hipHostFree(p));
    }
    const BufKind kind_;
    const size_t cap_;
    std::mutex mu_;
    std::multimap<std::pair<int, size_t>, void *> bufs_;  // (device, bucket) -> idle buffer
    size_t cached_ = 0;
};

BufCache &dev_cache() {
    static BufCache *c = new BufCache(kBufDevice, size_t(2) << 30);  // never destroyed
    return *c;
}
BufCache &pin_cache() {
    static BufCache *c = new BufCache(kBufPinned, size_t(1) << 30);
    return *c;
}
BufCache &map_cache() {  // pinned, mapped into the device address space, coherent
    static BufCache *c = new BufCache(kBufMapped, size_t(512) << 20);
    return *c;
}

// ---------------------------------------------------------------- holders
// One allocation of a BufCache.  It remembers its cache, device and byte count, so the
// release (explicit, on re-acquire, or when the holder dies) cannot disagree with the
// acquire.  As with BufCache::release, the buffer must be idle by then.  A mapped holder
// (map_cache()) also carries the buffer's device alias.
class Buf {
  public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) {
            release();
            cache_ = o.cache_, dev_ = o.dev_, bytes_ = o.bytes_, p_ = o.p_, alias_ = o.alias_;
            o.p_ = o.alias_ = nullptr;
            o.bytes_ = 0;
        }
        return *this;
    }
    ~Buf() { release(); }
    // >= bytes from cache c on device dev (the current device); false, and empty, if out of memory
    bool acquire(BufCache &c, int dev, size_t bytes) {
        release();
        if (!(p_ = c.acquire(dev, bytes))) return false;
        cache_ = &c, dev_ = dev, bytes_ = bytes;
        return true;
    }
    // ... mapped pinned, with its device alias; false, and empty, if either step fails
    bool acquire_mapped(int dev, size_t bytes) {
        if (acquire(map_cache(), dev, bytes) && hipHostGetDevicePointer(&alias_, p_, 0) == hipSuccess) return true;
        (void)hipGetLastError();
        release();
        return false;
    }
    void release() {
        if (p_) cache_->release(dev_, p_, bytes_);
        p_ = alias_ = nullptr;
        bytes_ = 0;
    }
    size_t bytes() const { return bytes_; }  // as acquired; 0 when empty
    explicit operator bool() const { return p_ != nullptr; }
    template <class T = uint8_t> T *get() const { return static_cast<T *>(p_); }
    template <class T = uint8_t> T *alias() const { return static_cast<T *>(alias_); }

  private:
    BufCache *cache_ = nullptr;
    int dev_ = -1;
    size_t bytes_ = 0;
    void *p_ = nullptr, *alias_ = nullptr;
};

// Two halves of a staging area with an event and a pending flag each: half h may be
// overwritten from the host once the work recorded behind its last use has completed.
struct HalfPipe {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};
    HalfPipe() = default;
    HalfPipe(const HalfPipe &) = delete;
    HalfPipe &operator=(const HalfPipe &) = delete;
    ~HalfPipe() { destroy(); }
    hipError_t create(unsigned flags) {  // (the events still missing)
        for (hipEvent_t &e : ev)
            if (!e)
                if (hipError_t rc = hipEventCreateWithFlags(&e, flags); rc != hipSuccess) return rc;
        return hipSuccess;
    }
    void destroy() {
        for (hipEvent_t &e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        forget();
    }
    hipError_t wait(int h) {
        if (!pending[h]) return hipSuccess;
        const hipError_t rc = hipEventSynchronize(ev[h]);
        if (rc == hipSuccess) pending[h] = false;
        return rc;
    }
    hipError_t record(int h, hipStream_t s) {
        const hipError_t rc = hipEventRecord(ev[h], s);
        if (rc == hipSuccess) pending[h] = true;
        return rc;
    }
    hipError_t wait_all() {
        const hipError_t a = wait(0), b = wait(1);
        return a != hipSuccess ? a : b;
    }
    void forget() { pending[0] = pending[1] = false; }  // (the stream was synchronised)
};

// Nothing of a failed call may stay in flight: its earlier launches and copies may still
// read the object's staging and tile lists, which the next call overwrites from the host.
// Declared where a call starts to enqueue such work; every exit that did not dismiss()
// it -- a failed launch, any HIP_TRY -- synchronises the stream and clears the sticky
// error.  A success path keeps its own completion and dismisses: no second wait.
class InFlight {
  public:
    explicit InFlight(hipStream_t s, HalfPipe *pipe = nullptr) : s_(s), pipe_(pipe) {}
    InFlight(const InFlight &) = delete;
    InFlight &operator=(const InFlight &) = delete;
    ~InFlight() {
        if (!armed_) return;
        (void)hipStreamSynchronize(s_);
        (void)hipGetLastError();
        if (pipe_) pipe_->forget();
    }
    void dismiss() { armed_ = false; }

  private:
    hipStream_t s_;
    HalfPipe *pipe_;
    bool armed_ = true;
};

// What kind of memory p is: its device-usable address (device memory, or pinned /
// registered / managed host memory mapped into the device address space; NULL for
// pageable host memory), and whether the host may read it in place on return -- pinned
// or managed memory, so a result the kernel wrote there needs the system-scope release.
struct PtrKind {
    void *dev = nullptr;
    bool host = false;
    bool known = false;  // the query succeeded
    bool device_memory() const { return dev && !host; }
};
PtrKind classify(const void *p) {
    PtrKind k;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return k;
    }
    k.known = true;
    k.host = at.type == hipMemoryTypeHost || at.type == hipMemoryTypeManaged;
    if (k.host || at.type == hipMemoryTypeDevice) k.dev = at.devicePointer;
    return k;
}
void *device_view_of(const void *p) { return classify(p).dev; }

// Any of the n outputs in host memory (pinned / registered / managed): the synchronous call
// that wrote them then waits with host_results (stream_wait).  Unknown: be safe.
bool any_host_memory(uint8_t *const *out, int n) {
    for (int i = 0; out && i < n; ++i) {
        if (!out[i]) continue;
        const PtrKind k = classify(out[i]);
        if (!k.known || k.host) return true;
    }
    return false;
}

// ---------------------------------------------------------------- pattern cache
struct PatEntry {
    std::string key;
    int dev = 0;
    uint8_t *d = nullptr, *h = nullptr;  // device copy, pinned mirror (bucket bytes each)
    hipEvent_t up = nullptr;             // recorded behind the upload
    std::atomic<bool> up_done{false};  // (read without the lock by the region-multiply memo)
    bool captured = false;  // used inside a stream capture: never evicted
    int pins = 0;           // launches between pattern_get and pattern_done (under mu)
    std::list<PatEntry *>::iterator lru;
};

struct PatCache {
    std::mutex mu;
    std::unordered_map<std::string, PatEntry *, KeyHash> map;
    std::list<PatEntry *> lru;  // front = most recent
    size_t bytes = 0;
    uint64_t evictions = 0, uploads = 0;
};
// Never destroyed (like the buffer caches): entries stay reachable to the end, and no
// static destructor races a thread still launching at process exit.
PatCache *const g_pat = new PatCache[64];

std::atomic<int> g_pat_max_entries{[] {
    const char *e = getenv("CEC_PATTERN_CACHE_ENTRIES");
    return e && *e ? std::max(1, atoi(e)) : 4096;
}()};
constexpr size_t kPatMaxBytes = size_t(64) << 20;

// hipDeviceSynchronize before device memory that queued launches may read is reused.
// Relaxed capture mode: a device-wide wait is an "unsafe" call while any thread captures
// in global mode, and would be refused (and invalidate that capture) otherwise.
bool device_sync_for_reuse() {
    RelaxedCapture relax;
    if (hipDeviceSynchronize() == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

void pat_free(PatEntry *e) {
    dev_cache().release(e->dev, e->d, e->key.size());
    pin_cache().release(e->dev, e->h, e->key.size());
    if (e->up) (void)hipEventDestroy(e->up);
    delete e;
}

// Evict least recently used entries (not captured, not pinned) until `need` more bytes
// and `more` more entries fit, plus an eighth of the limit so that evictions come in
// batches.  An entry's tables may still be read by launches on any stream, some of
// which may have been destroyed since (a destroyed stream's handle must not be touched:
// hipStreamSynchronize on one crashes, tools/stream_probe.hip), so one device-wide
// synchronisation covers a whole batch.  With the default limit of 4096 sets a server
// with a fixed set of codes and masks never evicts.
void pat_evict(PatCache &c, size_t need, size_t more = 1) {
    const size_t limit = static_cast<size_t>(g_pat_max_entries.load());
    auto over = [&](size_t slack) {
        return c.map.size() + more + slack > limit || c.bytes + need > kPatMaxBytes;
    };
    if (!over(0)) return;
    const size_t slack = limit / 8;
    std::vector<PatEntry *> victims;
    size_t n = c.map.size(), bytes = c.bytes;
    for (auto it = c.lru.end(); it != c.lru.begin();) {
        --it;
        PatEntry *e = *it;
        if (e->captured || e->pins) continue;  // (a pinned entry is being launched with)
        if (!(n + more + slack > limit || bytes + need > kPatMaxBytes)) break;
        victims.push_back(e);
        --n;
        bytes -= cache_bucket(e->key.size());
    }
    if (victims.empty()) return;
    // Every launch that may read a victim has completed -- or nothing is freed: a refused
    // or failed synchronisation (another thread capturing in global mode; a faulted
    // kernel) keeps the victims, since a launch still queued may read their tables.
    if (!device_sync_for_reuse()) return;
    for (PatEntry *e : victims) {
        c.bytes -= cache_bucket(e->key.size());
        c.map.erase(e->key);
        c.lru.erase(e->lru);
        ++c.evictions;
        pat_free(e);
    }
}

// Device copy of the tables `key` for a launch on stream s; *entry receives the cache
// entry, pinned against eviction until pattern_done.
int pattern_get(int dev, std::string &&key, hipStream_t s, PatEntry **entry) {
    PatCache &c = g_pat[dev];
    const bool capturing = stream_capturing(s);
    // event queries / waits and allocation below are "unsafe" calls for a thread that
    // captures in global mode: they would invalidate the capture
    RelaxedCapture relax(capturing);
    std::lock_guard<std::mutex> lk(c.mu);
    auto it = c.map.find(key);
    PatEntry *e = nullptr;
    if (it != c.map.end()) {
        e = it->second;
        c.lru.splice(c.lru.begin(), c.lru, e->lru);
    } else {
        // (no eviction while capturing: it synchronises streams, possibly this one)
        if (!capturing) pat_evict(c, cache_bucket(key.size()));
        e = new PatEntry;
        e->dev = dev;
        e->d = static_cast<uint8_t *>(dev_cache().acquire(dev, key.size()));
        e->h = static_cast<uint8_t *>(pin_cache().acquire(dev, key.size()));
        if (!e->d || !e->h || hipEventCreateWithFlags(&e->up, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            e->key = key;  // sizes for the release
            pat_free(e);
            return fail(CEC_ENOMEM, "coefficient tables: %zu bytes", key.size());
        }
        memcpy(e->h, key.data(), key.size());
        // Upload on the caller's stream, not a library stream: one more HIP stream in the
        // process (a hardware queue, even idle) measured the rotating decode 2.5 % slower
        // (DESIGN.md).  Inside a capture the upload must happen now, outside the graph:
        // through a temporary stream, waited for on the host.
        hipStream_t us = s, tmp = nullptr;
        if (capturing && hipStreamCreateWithFlags(&tmp, hipStreamNonBlocking) == hipSuccess) us = tmp;
        bool ok = hipMemcpyAsync(e->d, e->h, key.size(), hipMemcpyHostToDevice, us) == hipSuccess &&
                  hipEventRecord(e->up, us) == hipSuccess;
        if (tmp) {
            ok = ok && hipStreamSynchronize(tmp) == hipSuccess;
            (void)hipStreamDestroy(tmp);
            e->up_done = ok;
        } else if (capturing) {
            ok = false;  // no temporary stream: refuse rather than capture the upload
        }
        if (!ok) {
            (void)hipGetLastError();
            e->key = key;
            pat_free(e);
            return fail(CEC_EHIP, "coefficient tables: upload");
        }
        ++c.uploads;
        e->key = std::move(key);
        c.lru.push_front(e);
        e->lru = c.lru.begin();
        c.map.emplace(e->key, e);
        c.bytes += cache_bucket(e->key.size());
    }
    if (!e->up_done && capturing) {
        // No event call may touch a capturing stream (the upload may have been queued on
        // this very stream before the capture began): upload the same bytes again through
        // a temporary stream, now, outside the graph.  Rewriting identical bytes is benign
        // if the first upload is still in flight.
        hipStream_t tmp = nullptr;
        if (hipStreamCreateWithFlags(&tmp, hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            return fail(CEC_EHIP, "coefficient tables: upload stream during capture");
        }
        const bool ok = hipMemcpyAsync(e->d, e->h, e->key.size(), hipMemcpyHostToDevice, tmp) == hipSuccess &&
                        hipStreamSynchronize(tmp) == hipSuccess;
        (void)hipStreamDestroy(tmp);
        if (!ok) {
            (void)hipGetLastError();
            return fail(CEC_EHIP, "coefficient tables: upload during capture");
        }
        e->up_done = true;
    } else if (!e->up_done) {
        if (hipEventQuery(e->up) == hipSuccess) {
            e->up_done = true;
        } else if (hipStreamWaitEvent(s, e->up, 0) != hipSuccess) {
            return fail(CEC_EHIP, "coefficient tables: stream wait");
        }
        (void)hipGetLastError();
    }
    if (capturing) e->captured = true;
    ++e->pins;  // until pattern_done: no other thread may evict it before its launch is noted
    *entry = e;
    return CEC_OK;
}

// The launch that pattern_get pinned `e` for has been enqueued and noted on its stream.
void pattern_done(PatEntry *e) {
    std::lock_guard<std::mutex> lk(g_pat[e->dev].mu);
    --e->pins;
}

}  // namespace

// ---------------------------------------------------------------- C-ABI
CEC_API int cec_cache_get_info(cec_cache_info *out) {
    if (!out) return fail(CEC_EINVAL, "cec_cache_get_info: out is NULL");
    int dev;
    if (int r = current_device(&dev)) return r;
    PatCache &c = g_pat[dev];
    std::lock_guard<std::mutex> lk(c.mu);
    out->pattern_entries = c.map.size();
    out->pattern_bytes = c.bytes;
    out->pattern_uploads = c.uploads;
    out->pattern_evictions = c.evictions;
    out->pattern_entry_limit = static_cast<uint64_t>(g_pat_max_entries.load());
    out->device_cached_bytes = dev_cache().cached();
    out->pinned_cached_bytes = pin_cache().cached() + map_cache().cached();
    return CEC_OK;
}

CEC_API int cec_cache_set_pattern_limit(int entries) {
    if (entries < 1) return fail(CEC_EINVAL, "cec_cache_set_pattern_limit: %d", entries);
    g_pat_max_entries.store(entries);
    int dev;
    if (int r = current_device(&dev)) return r;
    PatCache &c = g_pat[dev];  // shrink this device's cache now (others at their next upload)
    std::lock_guard<std::mutex> lk(c.mu);
    pat_evict(c, 0, 0);
    return CEC_OK;
}

namespace {
// Evict every evictable coefficient-table set of one device's cache (waits for their
// streams), then free the idle buffers.
void trim_device_tables(int dev) {
    PatCache &c = g_pat[dev];
    std::lock_guard<std::mutex> lk(c.mu);
    if (c.lru.empty()) return;
    if (!device_sync_for_reuse()) return;  // (see pat_evict: no stream handle is touched)
    for (auto it = c.lru.begin(); it != c.lru.end();) {
        PatEntry *e = *it;
        if (e->captured || e->pins) {
            ++it;
            continue;
        }
        c.bytes -= cache_bucket(e->key.size());
        c.map.erase(e->key);
        it = c.lru.erase(it);
        pat_free(e);
    }
}

// At process exit, before the HIP runtime's own teardown (this handler is registered
// after the runtime initialised, so it runs first): give every idle cached buffer and
// table back.  Holding pinned and device memory across exit made LeakSanitizer's exit
// scan hang (tools/asan.sh), and a clean exit is what a server's shutdown expects.
void exit_trim() {
    // No stream handle is touched here (the streams an entry was used on may be gone by
    // now): each device with cached state is synchronised as a whole instead, which at
    // exit is what a server's shutdown does anyway.
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (int d = 0; d < 64; ++d) {
        PatCache &c = g_pat[d];
        std::lock_guard<std::mutex> lk(c.mu);
        if (c.lru.empty()) continue;
        if (hipSetDevice(d) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            (void)hipGetLastError();
            continue;  // the device is gone or faulted: leave its memory to the process
        }
        for (auto it = c.lru.begin(); it != c.lru.end();) {
            PatEntry *e = *it;
            if (e->captured || e->pins) {  // a graph may still be replayed by a late thread
                ++it;
                continue;
            }
            c.bytes -= cache_bucket(e->key.size());
            c.map.erase(e->key);
            it = c.lru.erase(it);
            pat_free(e);
        }
    }
    (void)hipSetDevice(cur);
    dev_cache().trim();  // idle by definition: only finished work's buffers are cached
    pin_cache().trim();
    map_cache().trim();
}

void register_exit_trim() {
    static std::once_flag once;
    std::call_once(once, [] { std::atexit(exit_trim); });
}
}  // namespace

CEC_API int cec_cache_trim(void) {
    int dev;
    if (int r = current_device(&dev)) return r;
    trim_device_tables(dev);
    dev_cache().trim();
    pin_cache().trim();
    map_cache().trim();
    return CEC_OK;
}
