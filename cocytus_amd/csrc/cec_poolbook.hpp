// cec_poolbook.hpp -- the recovery pool's host bookkeeping that touches no device:
// what a request's mask asks of its leader, when a request is ready to be solved, the
// all-or-nothing check of a batch of parity residuals, the stream slots of a flush and
// the key of a flush pattern.  Plain C++ (no HIP), included by cec_pool.inc and, as
// shipped, by tests/drain_c/pool_book_main.cpp, which runs it under ASan + UBSan.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace poolbook {

constexpr int kMaxK = 16, kMaxM = 8;  // CEC_MAX_K, CEC_MAX_M (asserted in cec_pool.inc)
constexpr int kStreams = 48;          // kMaxStreams
constexpr int kInputs = 16;           // kPatN
constexpr int kOutputs = 4;           // kPatL

// A recovery mask names k lids (mask_ok): the data lids that answer and as many parities
// as data lids are lost.
inline uint32_t data_lids(int k, uint32_t mask) { return mask & ((1u << k) - 1); }
inline uint32_t parity_lids(int k, uint32_t mask) { return mask & ~((1u << k) - 1); }
inline int n_lost(int k, uint32_t mask) { return __builtin_popcount(parity_lids(k, mask)); }
// The parities whose residuals the leader `self` must be given: the mask's others.
inline uint32_t needed(int k, int self, uint32_t mask) { return parity_lids(k, mask) & ~(1u << self); }

// What the checks read of a request.
struct Req {
    bool live = false;
    uint32_t mask = 0;
    uint32_t contributed = 0;  // data lids applied or queued
    uint32_t given = 0;        // parity lids whose residual was given
};

// check_recovery_1st_completeness: every data lid of the mask applied or queued.
inline bool complete(int k, const Req &r) {
    return r.live && (r.contributed & data_lids(k, r.mask)) == data_lids(k, r.mask);
}
// ... and every other participating parity's residual given.  A single loss needs none:
// ready == complete.
inline bool ready(int k, int self, const Req &r) {
    return complete(k, r) && (r.given & needed(k, self, r.mask)) == needed(k, self, r.mask);
}

// The ids with something for the next flush, each at most once: `flag` is the request's
// own "in the queue" mark.  A flush clears queue and marks; a request that ends while
// marked is taken out (dequeue), so an id reused by the next begin -- which starts
// unmarked -- cannot enter twice.
inline void enqueue(std::vector<int> &queue, bool &flag, int id) {
    if (!flag) queue.push_back(id);
    flag = true;
}
inline void dequeue(std::vector<int> &queue, bool &flag, int id) {
    if (flag) queue.erase(std::remove(queue.begin(), queue.end(), id), queue.end());
    flag = false;
}

enum Refusal {
    kAccepted = 0,
    kNotLive,     // no such request
    kNotParity,   // the lid is no parity of the request's mask
    kSelf,        // the pool's own parity: its residual is R
    kTwice,       // that parity's residual was given before
    kSingleLoss,  // a single-loss request takes none
    kPairTwice,   // batch: a (request, parity) pair listed twice
};

inline Refusal check_residual(int k, int m, int self, const Req &r, int lid) {
    if (!r.live) return kNotLive;
    if (n_lost(k, r.mask) < 2) return kSingleLoss;  // (its one parity is the pool's own)
    if (lid == self) return kSelf;
    if (lid < k || lid >= k + m || !(r.mask & (1u << lid))) return kNotParity;
    if (r.given & (1u << lid)) return kTwice;
    return kAccepted;
}

// Every entry of a batch checked before any is queued.  req_of(id) -> Req (live = false for
// an id out of range).  *bad = the first refused entry.
template <class Lookup>
Refusal check_residuals(int k, int m, int self, const int *ids, const int *lids, int n, Lookup req_of, int *bad) {
    std::vector<std::pair<int, int>> seen;
    seen.reserve(n > 0 ? n : 0);
    for (int i = 0; i < n; ++i) {
        if (Refusal why = check_residual(k, m, self, req_of(ids[i]), lids[i])) {
            if (bad) *bad = i;
            return why;
        }
        seen.emplace_back(ids[i], lids[i]);
    }
    std::vector<std::pair<int, int>> sorted = seen;
    std::sort(sorted.begin(), sorted.end());
    auto dup = std::adjacent_find(sorted.begin(), sorted.end());
    if (dup != sorted.end()) {
        if (bad) *bad = static_cast<int>(std::find(seen.begin(), seen.end(), *dup) - seen.begin());
        return kPairTwice;
    }
    return kAccepted;
}

// The stream slots of a flush.  Its patterns outlive the call (the pool's table is append-
// only) with the slots baked in, so a slot is a function of (k, m) alone:
//
//   0            P, this parity's arena
//   1            R, the residuals
//   2 .. 2+k     Q_j, data lid j's reply staging
//   2+k .. 2+2k  a flush_solve: the arena of data lid j; a flush_solve_host: host output
//                plane x in slot 2+k+x (x-th lost lid, x < n <= min(k, m)).  One flush has
//                arenas or host planes, never both, so they share the slots; the pattern
//                key carries to_host.
//   2+2k .. +m   G_p, the staging of parity k+p's given residuals (the own parity's slot
//                stays empty)
//
// 2 + 2k + m = 42 at k = 16, m = 8, within the kernels' 48.
struct FlushSlots {
    int k, m;
    int parity() const { return 0; }
    int residual() const { return 1; }
    int reply(int j) const { return 2 + j; }
    int out(int j) const { return 2 + k + j; }
    int given(int parity_lid) const { return 2 + 2 * k + (parity_lid - k); }
    int count() const { return 2 + 2 * k + m; }
};
static_assert(2 + 2 * kMaxK + kMaxM <= kStreams, "a flush's streams at k = 16, m = 8");

// The inputs of a fused flush pattern: P or R, the queued replies (at most the k - n data
// lids of the mask), the n - 1 given residuals: at most k <= kInputs.
inline int flush_inputs(int queued_replies, int n) { return 1 + queued_replies + (n - 1); }
static_assert(1 + (kMaxK - 1) + (1 - 1) <= kInputs && 1 + (kMaxK - kMaxM) + (kMaxM - 1) <= kInputs, "k inputs");
// ... and its outputs: R' if anything is folded, and the n rebuilt shards.  One launch
// holds kOutputs, so the flush's own launch solves n <= 3; more are solved behind it.
constexpr int kFusedLosses = kOutputs - 1;

// The key of a flush pattern: the queued data lids and the first touch decide the fold;
// a request solved in the same launch adds its whole mask (which lids are lost AND which
// parities' residuals come in, with their inverse) and where the shards go.  Requests not
// solved share one pattern per (queued, touch) whatever their mask.
// At most 2^k * 2 fold-only patterns, and per mask of <= 3 losses 2^(k-n) * 2 * 2
// (queued subsets of its k - n data lids, +1 for the residual-only pattern; touch; to_host).
inline uint64_t flush_key(uint32_t queued, bool touch, bool solved, uint32_t mask, bool to_host) {
    return static_cast<uint64_t>(queued & 0xFFFFu) | (touch ? 1ull << 16 : 0) |
           (solved ? (1ull << 17) | (to_host ? 1ull << 18 : 0) | (static_cast<uint64_t>(mask) << 32) : 0);
}

// The launches of an explicit solve of requests losing up to n_max shards.
inline int solve_launches(int n_max) { return (n_max + kOutputs - 1) / kOutputs; }

}  // namespace poolbook
