// cec_hostplan.hpp -- the host-side planning shared by the ops that take their work from
// host memory: the parity drain (cec_drain.inc), cec_region_multiply_batch
// (cec_hostbatch.inc), the recovery pool's fold_updates (cec_pool.inc) and the recovery
// sessions' HostStager (cec_recovery.inc).
//
// Standard library and cocytus_ec.h only -- no HIP type, no error reporting -- so the
// CPU tests (tests/drain_c) include this very file under ASan + UBSan.
//   PackPool / split_copy   persistent host threads; a list of copies split by bytes
//   radix_sort              (key, index) pairs by key
//   colour_intervals        start-sorted intervals into overlap-free waves
//   overlap_waves           the drainer's waves of a batch of updates
//   inside_area / split_by_area   a drainer batch against the drainer's own staging area
//   Hb* / hb_cluster_waves  the host batch's pieces, clusters and waves
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/cocytus_ec.h"

namespace cec {

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

inline int pack_threads() {
    if (const char *e = getenv("CEC_PACK_THREADS")) return std::max(1, atoi(e));
    const unsigned hw = std::thread::hardware_concurrency();
    return static_cast<int>(std::max(1u, std::min(8u, hw / 2)));
}

struct CopyItem {
    uint8_t *dst;
    const uint8_t *src;
    size_t len;
};

// Copies through the pack pool: thread t takes bytes [t*B/T, (t+1)*B/T) of the list.
// Lists of fewer than min_parallel bytes stay on the caller's thread (no wake-up).
inline void split_copy(PackPool *pool, const CopyItem *items, size_t n, size_t min_parallel) {
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) total += items[i].len;
    if (!pool || pool->size() == 1 || total < min_parallel) {
        for (size_t i = 0; i < n; ++i)
            if (items[i].len) memcpy(items[i].dst, items[i].src, items[i].len);
        return;
    }
    std::vector<size_t> prefix(n + 1, 0);
    for (size_t i = 0; i < n; ++i) prefix[i + 1] = prefix[i] + items[i].len;
    const int T = pool->size();
    pool->run([&](int t) {
        const size_t lo = total * t / T, hi = total * (t + 1) / T;
        if (lo >= hi) return;
        size_t i = std::upper_bound(prefix.begin(), prefix.end(), lo) - prefix.begin() - 1;
        for (size_t pos = lo; pos < hi && i < n; ++i) {
            const CopyItem &c = items[i];
            const size_t a = pos - prefix[i], b = std::min(c.len, hi - prefix[i]);
            if (b > a) memcpy(c.dst + a, c.src + a, b - a);
            pos = prefix[i] + b;
        }
    });
}
inline void split_copy(PackPool *pool, const std::vector<CopyItem> &items, size_t min_parallel) {
    split_copy(pool, items.data(), items.size(), min_parallel);
}

// (key, index) pairs sorted by key, equal keys by index: LSD radix sort, 11-bit digits,
// digits on which every key agrees skipped (an 8 GiB arena: at most 3 passes; host
// addresses of one batch differ in their low ~40 bits: <= 4).  For 65,536 shuffled keys it
// took 1.1 ms where std::sort through the index took 5.7 on the build host.
inline void radix_sort(std::vector<std::pair<uint64_t, int>> &a) {
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

// Greedy colouring of n intervals given in start order: span(i) = [first, second) of the
// i-th, set_wave(i, w) receives its wave = the lowest wave with no overlapping member.
// Sorted sweep with a min-heap of (end, wave) of the open intervals and the list of waves
// they gave back.  An empty interval takes a wave and frees it at once.  Returns the
// number of waves (>= 1), which for non-empty intervals is their deepest overlap.
template <class Span, class SetWave>
int colour_intervals(size_t n, Span span, SetWave set_wave) {
    std::vector<std::pair<uint64_t, int>> open;  // min-heap on end
    std::vector<int> free_waves;
    int nw = 0;
    auto cmp = [](const std::pair<uint64_t, int> &a, const std::pair<uint64_t, int> &b) {
        return a.first > b.first;
    };
    for (size_t i = 0; i < n; ++i) {
        const std::pair<uint64_t, uint64_t> iv = span(i);
        while (!open.empty() && open.front().first <= iv.first) {
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
        set_wave(i, w);
        if (iv.second > iv.first) {
            open.emplace_back(iv.second, w);
            std::push_heap(open.begin(), open.end(), cmp);
        } else {
            free_waves.push_back(w);
        }
    }
    return std::max(nw, 1);
}

// The drainer's waves: colouring of [addr, addr+len) over the updates sorted by arena
// address.  When no two updates overlap (the usual batch: distinct values), one linear
// pass over the sorted order proves it and every update is in wave 0.  Returns the number
// of waves; wave[i] is update i's.
inline int overlap_waves(const cec_host_update *u, int n, std::vector<int> &wave) {
    std::vector<std::pair<uint64_t, int>> byaddr(n);
    for (int i = 0; i < n; ++i) byaddr[i] = {u[i].addr, i};
    radix_sort(byaddr);  // (the colouring runs before the pack path can start)
    wave.assign(n, 0);
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
    return colour_intervals(
        byaddr.size(),
        [&](size_t i) {
            const cec_host_update &v = u[byaddr[i].second];
            return std::pair<uint64_t, uint64_t>(v.addr, v.addr + v.len);
        },
        [&](size_t i, int w) { wave[byaddr[i].second] = w; });
}

// A host buffer [b, b + len) against an area [base, base + cap), compared as integers (the
// two need not be one object): wholly inside it; sharing at least one byte with it.
inline bool inside_area(const void *b, size_t len, const void *base, size_t cap) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(b), a = reinterpret_cast<uintptr_t>(base);
    return p >= a && len <= cap && p - a <= cap - len;
}
inline bool meets_area(const void *b, size_t len, const void *base, size_t cap) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(b), a = reinterpret_cast<uintptr_t>(base);
    return len && p < a + cap && p + len > a;
}

// The two parts of a drainer batch that mixes diffs received in the staging area with diffs
// elsewhere: `in` takes the non-empty updates wholly inside [base, base + cap), `rest` every
// other non-empty one (a buffer that only partly lies in the area included), cut into pieces
// of at most `piece` bytes.  Both keep the list order; [*lo, *hi) receives the span of the
// area that `in` uses.
inline void split_by_area(const cec_host_update *u, int n, const void *base, size_t cap, uint32_t piece,
                          std::vector<cec_host_update> &in, std::vector<cec_host_update> &rest, uint64_t *lo,
                          uint64_t *hi) {
    in.clear();
    rest.clear();
    *lo = UINT64_MAX, *hi = 0;
    for (int i = 0; i < n; ++i) {
        if (!u[i].len) continue;
        const uint8_t *b = static_cast<const uint8_t *>(u[i].buf);
        if (inside_area(b, u[i].len, base, cap)) {
            const uint64_t at = reinterpret_cast<uintptr_t>(b) - reinterpret_cast<uintptr_t>(base);
            *lo = std::min<uint64_t>(*lo, at);
            *hi = std::max<uint64_t>(*hi, at + u[i].len);
            in.push_back(u[i]);
            continue;
        }
        for (uint32_t o = 0; o < u[i].len; o += std::min(piece, u[i].len - o))
            rest.push_back(cec_host_update{b + o, u[i].addr + o, std::min(piece, u[i].len - o), u[i].src_lid});
    }
}

// ---------------------------------------------------------------- the host batch's plan
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
inline int hb_cluster_waves(std::vector<HbPiece> &pc, const int *ids, int count, bool *packed) {
    if (count == 1) {
        pc[ids[0]].wave = 0;
        *packed = pc[ids[0]].kind == kHbXor;
        return 1;
    }
    bool writes = false;
    for (int i = 0; i < count; ++i) writes |= pc[ids[i]].kind != kHbXor;
    *packed = true;  // (a multi-piece cluster: conservatively staged in)
    if (!writes)  // XOR accumulation commutes: greedy colouring (ids are sorted by dst start)
        return colour_intervals(
            static_cast<size_t>(count),
            [&](size_t i) {
                const HbPiece &p = pc[ids[i]];
                const uint64_t lo = reinterpret_cast<uintptr_t>(p.dst);
                return std::pair<uint64_t, uint64_t>(lo, lo + p.len);
            },
            [&](size_t i, int w) { pc[ids[i]].wave = w; });
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

}  // namespace cec
